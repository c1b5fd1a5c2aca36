// Kernel 1: all-vs-all / ref x query core+accessory distances on gfx950 (CDNA4).
//
// Replaces the hot loop of pp_sketchlib.queryDatabase [EXT] (call sites
// PopPUNK/sketchlib.py:528-537,:584-593); arithmetic per SURVEY.md 8a rows a3-a7.
//
// Mapping to the hardware (this is integer set-intersection: no MFMA anywhere):
//  * sketches are resident as [k][word][sample], so one bit-plane word of 256
//    consecutive samples is one contiguous 2-KB row;
//  * a bin-plane compare-and-accumulate is ONE v_bitop3_b32 per 32 bins per pair:
//        bits = bits & ~(ref ^ qry)            (truth table 0x90)
//    and a 64-bin block costs 28 v_bitop3 + 2 v_bcnt per pair (2400 VALU/pair);
//  * dist_kernel_v2 (the hot path, bbits = 14): an 8-wavefront workgroup owns a
//    256-ref x 32-query pair tile.  Per 64-bin block its 14 ref rows (28 KB) and
//    14 query rows (3.5 KB) are copied HBM/L2 -> LDS by global_load_lds_dwordx4
//    (LDS-DMA: no VGPR round trip), double-buffered so the copy of block b+1
//    runs under the compare of block b with ONE s_barrier per block.  Each lane
//    owns 4 refs (two ds_read_b128 per plane, conflict-free) x the wavefront's
//    4 queries (two broadcast ds_read_b128), i.e. a 4x4 register tile: every
//    operand is a VGPR (measured on MI355X: v_bitop3 with an SGPR operand issues
//    at ~4.2 clk, all-VGPR at ~2.8 clk; tools/ubench_valu.hip);
//  * dist_kernel (v1; generic bbits and A/B experiments): 64 refs per wavefront
//    staged through LDS, query words through the scalar unit (s_load_dwordx16)
//    as SGPR operands;
//  * per-k match counts live in a 2/3/4-dword shift register per pair whose low
//    field IS the running counter of the current k (PackW below); the full block
//    also issues the wave's four DMA pieces of the next block from inside its own
//    instruction stream; after the last k the lane regresses log J on k in fp64 (log J comes
//    from a device-built table indexed by (cluster pair, k, count): the count
//    is an integer in [0, nbins], so the table is exact, not an approximation),
//    then writes float2 rows -- consecutive lanes are consecutive refs, which
//    are consecutive rows in both PopPUNK row orders (utils.py:199-226);
//  * with MODE_MASK the lane applies the boundary instead (src/boundary.cpp:42-58)
//    and the wavefront's __ballot is stored as one uint64 of an edge bitmask.
#include <cstdlib>
#include <type_traits>

#include <mutex>

#include "ppk_internal.h"
#include "ppk_block_asm.inc"

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned __int128 u128;

// Per-pair record of the per-k match counts.
//  * integer packs (uint64 / u128; Pack96 = six 16-bit counts in three dwords): count k at bit
//    k * cnt_bits -- the generic-bbits kernel and the small-job regression pass;
//  * PackW<W>: W dwords used as ONE shift register by the LDS-DMA tile kernel.  The running count
//    of the current k lives in the low cnt_bits bits (v_bcnt accumulates straight into dword 0,
//    and a count never exceeds nbins < 2^cnt_bits, so it cannot carry into its neighbour); at the
//    start of the next k the whole register moves up by cnt_bits.  Count k therefore ends at bit
//    (nk - 1 - k) * cnt_bits.  There are no separate counter registers: the 16 pairs of a lane
//    need 16 * W VGPRs (32 for the default 5 k x 11 bits, 64 at the 128-bit limit), all of which
//    fit beside the instruction stream's fixed registers -- dwords, not 64-bit values, because
//    those would each need an even-aligned register pair.
struct Pack96 {
  uint32_t w0, w1, w2;
};
template <int W> struct PackW {
  uint32_t w[W];
};
template <typename P> __device__ __forceinline__ void pack_zero(P &pk) { pk = 0; }
__device__ __forceinline__ void pack_zero(Pack96 &pk) { pk.w0 = pk.w1 = pk.w2 = 0u; }
template <typename P> __device__ __forceinline__ void pack_put(P &pk, uint32_t c, int k, int bits) {
  pk |= (P)c << (bits * k);
}
__device__ __forceinline__ void pack_put(Pack96 &pk, uint32_t c, int k, int) {
  const uint32_t x = c << (16 * (k & 1));
  const int j = k >> 1;             // wave-uniform: selects, not indexed registers
  pk.w0 |= j == 0 ? x : 0u;
  pk.w1 |= j == 1 ? x : 0u;
  pk.w2 |= j == 2 ? x : 0u;
}
// pack_get(pack, k, cnt_bits, mask, nk)
template <typename P> __device__ __forceinline__ uint32_t pack_get(const P &pk, int k, int bits, uint32_t mask, int) {
  return (uint32_t)(pk >> (bits * k)) & mask;
}
__device__ __forceinline__ uint32_t pack_get(const Pack96 &pk, int k, int, uint32_t, int) {
  const int j = k >> 1;
  const uint32_t w = j == 0 ? pk.w0 : (j == 1 ? pk.w1 : pk.w2);
  return (w >> (16 * (k & 1))) & 0xffffu;
}
template <int W> __device__ __forceinline__ uint32_t pack_get(const PackW<W> &pk, int k, int bits, uint32_t mask, int nk) {
  const int pos = (nk - 1 - k) * bits;      // wave-uniform: the dword choice is a select
  const int j = pos >> 5;
  uint32_t lo = pk.w[0], hi = W > 1 ? pk.w[W > 1 ? 1 : 0] : 0u;
#pragma unroll
  for (int i = 1; i < W; ++i)
    if (j == i) {
      lo = pk.w[i];
      hi = i + 1 < W ? pk.w[i + 1 < W ? i + 1 : i] : 0u;
    }
  return __builtin_amdgcn_alignbit(hi, lo, pos & 31) & mask;
}
// two dwords: one 64-bit shift (the epilogue is free to hold the register as an aligned pair)
__device__ __forceinline__ uint32_t pack_get(const PackW<2> &pk, int k, int bits, uint32_t mask, int nk) {
  const uint64_t v = ((uint64_t)pk.w[1] << 32) | pk.w[0];
  return (uint32_t)(v >> ((nk - 1 - k) * bits)) & mask;
}

enum { MODE_DIST = 0, MODE_JACCARD = 1, MODE_COUNTS = 2, MODE_MASK = 3, MODE_KNN = 4, MODE_BGMM = 5, MODE_MASK_ROWS = 6,
       MODE_BGMM_ROWS = 7 };
// The two edge-bitmask modes: MODE_MASK applies the refine/threshold line (ppk_line_dist), MODE_BGMM the label of a
// fitted BGMM (ppk_bgmm_label; the model is read through the kernel's otherwise unused `out` pointer).  Everything
// but the per-pair predicate is shared; the predicate is a compile-time choice, so MODE_BGMM adds instantiations
// and leaves those of MODE_MASK as they were.
// MODE_MASK_ROWS / MODE_BGMM_ROWS: the same two modes, which also hand out the unscaled (core, accessory) row of every
// pair whose bit they set (rows_emit below; ppk_dist_edges_rows_dev).  Instantiations of their own again: the mask
// modes' kernels stay as they were.  Whole tiles of the plain packed kernels only (no k-split, no wide window, no strip
// tiles: the host plans none, ppk_edge_rows_fused).
constexpr bool ppk_is_rows(int mode) { return mode == MODE_MASK_ROWS || mode == MODE_BGMM_ROWS; }
constexpr bool ppk_is_mask(int mode) { return mode == MODE_MASK || mode == MODE_BGMM || ppk_is_rows(mode); }
constexpr bool ppk_is_bgmm(int mode) { return mode == MODE_BGMM || mode == MODE_BGMM_ROWS; }

// MODE_KNN (k nearest neighbours of every sample, straight from the tiles; self job: among the other samples,
// ref x query job: of every query among the refs AND of every ref among the queries, queries numbered
// n_ref + q): a pair's distance is a CANDIDATE for both of its samples' neighbour lists.  Two filters keep the candidate
// stream small without ever dropping a true neighbour (keys are (distance bits, other sample):
// distances are >= 0, so their bits order like the values, and the sample index breaks ties exactly
// like the reference's stable sort by distance):
//  * local top-k: a tile holds 256 candidates for each of its 32 queries and 32 for each of its 256
//    refs; a candidate that is not among the k smallest keys of (a subset of) its sample's candidates
//    here cannot be among the k smallest overall;
//  * bounds: `thr[s]` is an upper bound of sample s's final k-th smallest distance -- the k-th
//    smallest of any k or more of its candidates is one -- lowered (atomicMin) by every tile that
//    holds enough of them; a candidate is emitted only if d <= thr[s] (<=: ties stay in play).
//    Bounds only ever tighten and a stale read is merely conservative, so tiles need no ordering.
// Out comes a superset of every true neighbour list: ~k (2 + ln(n/256) + ln(n/16)) candidates per
// sample instead of n.  Queries are handled by the wavefront that owns them (k rounds of wave-wide
// minimum extraction over its 4 x 64 registers); refs need all 32 queries of the tile, so the
// distances go through LDS (idle after the compare loop) and each thread ranks 16 of one ref's 32.
// One global atomic per workgroup reserves the tile's slice of the candidate arrays.
struct KnnState {
  unsigned long long count;   // candidates emitted (may exceed cap: the host then re-runs with more room)
  unsigned long long cap;     // capacity of the candidate arrays
  unsigned long long vals_off;   // byte offset of the uint64 value array behind the uint32 key array
  // uint32 thr[n] follows
};

// (internal) the one-launch k-split path could not get its scratch: the caller falls back to the tile kernel
constexpr int kNoKsplitScratch = -7001;

struct DistParams {
  size_t npad_r, npad_q;  // padded sample counts of the two resident arrays
  size_t n_ref;           // refs (lane axis)
  size_t q_begin, q_end;  // band of query rows
  size_t row_base;        // first distance row of the band
  size_t lut_kstride;     // nbins + 1
  size_t lut_cpstride;    // nk * (nbins + 1)
  size_t n_rtiles;        // ceil(n_ref / 64)
  size_t q_tile0;         // first query tile of the band (units of QT)
  int self, nk, s64, bbits;
  int cnt_bits;           // bits per packed count
  int n_clu;
  int random_correct;
  int slope, inclusive;   // MODE_MASK
  float x_max, y_max, scale_x, scale_y;
  // v2 MODE_DIST / MODE_MASK, self job with a ragged right edge: the first n_strip blocks of the grid are
  // "strip" tiles -- the last (n_ref mod 256) refs sit on the query axis against all smaller
  // samples on the lane axis (valid iff lane sample < strip sample); the rest are the triangle.
  unsigned n_strip;       // number of strip blocks (0 = none)
  unsigned strip_rt0;     // first lane tile of the strip (band start / 256)
  unsigned strip_r_tiles; // lane tiles the strip covers
  size_t strip_begin;     // first strip sample (= r_limit of the triangle part)
  size_t r_limit;         // triangle part: lane samples >= r_limit are left to the strip
  int xcd_map;            // 1: XCD-aware tile order (v2)
  unsigned xcd_shift;     // log2 of the device's XCD count (PpkGeometry: 3 on MI355X in SPX mode, 0 on one XCD)
  int lut32;              // the whole fit table is addressable with 32-bit byte offsets
  size_t lut_total;       // doubles in the log-J table; the (E, F) table of the fast path follows it
  int k_split;            // > 0: the KSPLIT instantiation (gridDim.y = nk * k_split: one k, or a half / quarter of one, per workgroup)
  size_t ks_rows;         // KSPLIT: rows of the band; its counts go to scratch k-major, [k][row]
  int ks_blocks;          // KSPLIT: 64-bin blocks one workgroup compares (s64 / k_split)
  unsigned ks_units;      // KSPLIT, fused fit: workgroups per tile (nk * k_split = gridDim.y)
  size_t ks_part_off;     // KSPLIT, fused fit: byte offset of the partial counts behind the tile counters
  unsigned *ks_tickets;   // KSPLIT, fused fit: one counter per tile (zero between launches)
  unsigned r_tiles, q_tiles;   // v2 tile grid
  unsigned n_strip_pad;        // n_strip rounded up to a multiple of 8 (keeps block % 8 = XCD for the rest)
  unsigned n_tiles;            // non-empty tiles of the triangle / rectangle part
  unsigned tiles_per_xcd;      // ceil(n_tiles / 8)
  int tri_m, tri_c0;           // self job: ref tile r pairs with clamp(tri_m * r + tri_c0, 0, q_tiles) query tiles
  int knn, knn_col;       // MODE_KNN: neighbours per sample, distance column (0 core, 1 accessory)
  int lds_table;          // interior tiles fit from the (E, F) table in LDS (option "lds_table"; 0: every tile takes the general statement -- same bits)
  int ablate;             // experiments build only (PPK_ABLATE): 1 skip epilogue, 2 skip compare, 4 skip DMA, 8 skip barriers, 64 skip the (E, F) table copy
  // WIDE instantiation (nk * cnt_bits > 128): the 128-bit count register holds wide_kpg k-mer lengths; when it is
  // full the workgroup parks it in its spill slot (see PackWide) and starts the next group from zero
  int wide_kpg;                    // k-mer lengths per group = 128 / cnt_bits (0: not a wide launch)
  int wide_groups;                 // ceil(nk / wide_kpg)
  unsigned wide_nslots;            // spill slots (a power of two, >= 2 x the workgroups a device can hold)
  unsigned *wide_bitmap;           // one bit per slot: taken (zero between launches)
  unsigned long long *wide_slots;  // [slot][group][32][512 threads] uint64
  int ext_adjust;         // [EXT] a4 gate (PpkConfig::ext_collision_adjust)
  int ext_skip;           // [EXT] a6: skip instead of truncate at J < 5/s (PpkConfig::ext_fit_skip)

  int kmers[PPK_MAX_NK];
  // dist_kernel_v2_rank only (appended: every field above keeps its offset).  Bit b of rank_short[k]: block b of k holds
  // at most 2^(P-1) distinct values per position, so plane P-1 of its codes is zero and the kernel compares P-1 planes
  // there (PpkCoding::less1; all zero with option "rank_short" 0).  The kernel reads word k at the end of k - 1, and
  // word nk after the last k: PPK_RANK_SHORT_WORDS > nk.
  unsigned rank_short[PPK_RANK_SHORT_WORDS];
  // the FOLD2 instantiations only: the event list of the two-holder pair (PpkCoding::d_list / d_off / rt)
  const uint16_t *fold2_ev;
  const unsigned *fold2_off;
  unsigned fold2_rt;
  // Bit b of fold2_six[k]: block b of k spans at most 2^6 codes, planes 6 and 7 are zero there and the kernel compares
  // 6 planes (PpkCoding::less2; every such bit is set in rank_short[k] too; all zero with "fold2_min_planes" 7).
  // Fetched where rank_short is.
  unsigned fold2_six[PPK_RANK_SHORT_WORDS];
  // MODE_MASK_ROWS / MODE_BGMM_ROWS only (appended: every field above keeps its offset).  rows_stage: float2 [rows_cap],
  // filled in the order the wavefronts reserve it; rows_base: parallel to the mask, the staging position of a word's
  // first row (written for the words with a bit); rows_count: positions reserved so far (zero before the first launch)
  float2 *rows_stage;
  unsigned long long *rows_base;
  unsigned long long *rows_count;
  unsigned long long rows_cap;
};

// With every k usable the least-squares fit is LINEAR in the log J_k with launch-constant weights:
//   slope = sum_k a_k log J_k,   intercept = sum_k b_k log J_k,
//   a_k = (nk x_k - sum x) / (nk sum x^2 - (sum x)^2),   b_k = (1 - a_k sum x) / nk,
// so 1 - e^slope = 1 - prod_k J_k^a_k: the table holds E = J^a_k and F = J^b_k per (k, count) and the
// fast path of the fit is nk look-ups and 2 (nk - 1) multiplications -- no sums, no exp.
struct FitCoef {
  double a[PPK_MAX_NK], b[PPK_MAX_NK];
};

// ---- small device helpers --------------------------------------------------

// a4: collision adjustment + observed Jaccard (integer part as in the source).  `adjust` is the
// [EXT] gate (PpkConfig::ext_collision_adjust): 0 = never in effect (upstream as recalled), 1 =
// applied when expected > 0.
__device__ __forceinline__ double jaccard_obs(uint32_t same, size_t s64, size_t bbits, int adjust) {
  const size_t maxnbits = s64 * 64;
  const size_t expected = maxnbits >> bbits;
  size_t inter = same;
  if (adjust && expected) {
    const size_t ret = same > expected ? same - expected : 0;
    inter = ret * maxnbits / (maxnbits - expected);
  }
  return (double)inter / (double)maxnbits;
}

// a5: observed_excess(obs, exp, 1)
__device__ __forceinline__ double observed_excess(double obs, double expd) {
  const double diff = obs > expd ? obs - expd : 0.0;
  return diff / (1.0 - expd);
}

// ---- layout + table kernels -------------------------------------------------

// [n][cols] -> [cols][npad] (cols = nk*words), padding samples zero-filled.
__global__ void __launch_bounds__(256)
transpose_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, size_t n,
                 size_t cols, size_t npad) {
  __shared__ uint64_t tile[32][33];
  const size_t c0 = (size_t)blockIdx.x * 32, s0 = (size_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const size_t s = s0 + i, c = c0 + tx;
    tile[i][tx] = (s < n && c < cols) ? in[s * cols + c] : 0ull;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const size_t c = c0 + i, s = s0 + tx;
    if (c < cols && s < npad) out[c * npad + s] = tile[tx][i];
  }
}

// LUT[(cr*C + cq)][k][count] = log J, or +1.0 when J < 5/nbins (the point and
// every later k are dropped from the fit; docs/sketching.rst:161-165).  Behind it, per entry, the
// pair (E, F) = (J^a_k, J^b_k) of the all-k-usable fast path (FitCoef), NaN where the log-J entry is
// the +1.0 marker: a NaN product sends the pair to the general fit.
__global__ void __launch_bounds__(256)
lut_kernel(double *__restrict__ lut, const float *__restrict__ rtab, int nk, int n_clu,
           size_t nbins, size_t s64, size_t bbits, int random_correct, int adjust, size_t total,
           const FitCoef coef) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const size_t per = nbins + 1;
  const uint32_t c = (uint32_t)(idx % per);
  const size_t k = (idx / per) % nk;
  const size_t cp = idx / (per * nk);
  double jr = 0.0;
  if (random_correct) jr = (double)rtab[(k * n_clu + cp / n_clu) * n_clu + cp % n_clu];
  const double j = observed_excess(jaccard_obs(c, s64, bbits, adjust), jr);
  const double tol = 5.0 / (double)nbins;
  const bool usable = !(j < tol);
  const double y = usable ? log(j) : 1.0;
  lut[idx] = y;
  double *ef = lut + total + 2 * idx;
  ef[0] = usable ? exp(coef.a[k] * y) : __builtin_nan("");
  ef[1] = usable ? exp(coef.b[k] * y) : __builtin_nan("");
}

// ---- the pair-tile kernel ----------------------------------------------------

// e^x for x <= 0 (the fitted slope / intercept), fp64: n = rint(x log2 e), r = x - n ln 2 in two
// parts, degree-11 Taylor polynomial on |r| <= 0.347 (truncation 6e-15 relative), scaled by 2^n.
// A third of the instructions of the library exp (no overflow / NaN / +x handling needed here);
// the result is rounded to float32 by the caller, which this error changes for ~2 in 1e7 values.
constexpr double kExpC[12] = {2.50521083854417187751e-08,   // 1/11!
                              2.75573192239858906526e-07,   // 1/10!
                              2.75573192239858906526e-06,   // 1/9!
                              2.48015873015873015873e-05,   // 1/8!
                              1.98412698412698412698e-04,   // 1/7!
                              1.38888888888888888889e-03,   // 1/6!
                              8.33333333333333333333e-03,   // 1/5!
                              4.16666666666666666667e-02,   // 1/4!
                              1.66666666666666666667e-01,   // 1/3!
                              0.5, 1.0, 1.0};

// N values in lock-step, so that every coefficient is materialised once per N evaluations (64-bit
// constants cannot be literals of an fp64 instruction; one at a time the compiler re-creates the
// twelve of them for every call).  Identical arithmetic per element whatever N is.
template <int N>
__device__ __forceinline__ void exp_nonpos_n(const double (&x)[N], double (&e)[N]) {
  double n[N], r[N], q[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    n[i] = __builtin_rint(x[i] * 1.4426950408889634074);
    r[i] = __builtin_fma(n[i], -6.93147180369123816490e-01, x[i]);
    r[i] = __builtin_fma(n[i], -1.90821492927058770002e-10, r[i]);
    q[i] = kExpC[0];
  }
#pragma unroll
  for (int c = 1; c < 12; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) q[i] = __builtin_fma(q[i], r[i], kExpC[c]);
#pragma unroll
  for (int i = 0; i < N; ++i) e[i] = __builtin_ldexp(q[i], (int)n[i]);
}

__device__ __forceinline__ double exp_nonpos(double x) {
  const double xs[1] = {x};
  double es[1];
  exp_nonpos_n<1>(xs, es);
  return es[0];
}

// a6 for one pair, fp64.  Every caller evaluates the SAME expressions in the same order, so a
// pair's result does not depend on which kernel, tile, band or wavefront computed it:
//  * every k usable (the overwhelmingly common case): core = 1 - prod_k E_k, accessory =
//    1 - prod_k F_k, products taken in k order from the (E, F) table (FitCoef) -- a NaN entry marks
//    a k below the 5/nbins floor;
//  * otherwise OLS of log J on k over the usable points (the leading run, or with ext_skip every
//    usable k), sums in k order with sxy as an fma, then 1 - e^x with exp_nonpos.
template <typename PackT, typename ParamsT>
__device__ __forceinline__ void fit_general(const PackT &pk, const double *__restrict__ lutp,
                                            const ParamsT &p, float &core, float &acc,
                                            bool &failed) {
  const uint32_t cmask = (1u << p.cnt_bits) - 1u;
  double sx = 0.0, sxx = 0.0, sy = 0.0, sxy = 0.0;
  int n = 0;
  bool open = true;
  for (int k = 0; k < p.nk; ++k) {
    const uint32_t c = pack_get(pk, k, p.cnt_bits, cmask, p.nk);
    const double y = lutp[(size_t)k * p.lut_kstride + c];
    // [EXT] truncate at (default) / skip the k below the floor.  `!(y > 0)`, not `y <= 0`: a NaN Jaccard (a random-match
    // entry of exactly 1: 0 / 0 in observed_excess) is not "below the floor" -- upstream's `jaccard < tolerance` is
    // false for it -- so the point stays, the sums turn NaN and both distances come out 0, not counted as failed
    open = (p.ext_skip || open) && !(y > 0.0);
    if (open) {
      const double x = (double)p.kmers[k];
      sx += x;
      sxx += x * x;
      sy += y;
      sxy = __builtin_fma(x, y, sxy);
      ++n;
    }
  }
  if (n < 2) {
    core = 0.0f;
    acc = 0.0f;
    failed = true;
    return;
  }
  const double dn = (double)n;
  const double slope = (dn * sxy - sx * sy) / (dn * sxx - sx * sx);
  const double icpt = (sy - slope * sx) / dn;
  core = slope < 0.0 ? (float)(1.0 - exp_nonpos(slope)) : 0.0f;
  acc = icpt < 0.0 ? (float)(1.0 - exp_nonpos(icpt)) : 0.0f;
  failed = false;
}

// (1 - prod E, 1 - prod F) clamped at 0: the fast path's last step, shared by every caller
__device__ __forceinline__ void fit_finish(double pe, double pf, float &core, float &acc) {
  core = pe < 1.0 ? (float)(1.0 - pe) : 0.0f;
  acc = pf < 1.0 ? (float)(1.0 - pf) : 0.0f;
}

// cp_off: offset (in entries) of the pair's cluster-pair block: its log J at lut[cp_off + ...], its
// (E, F) pairs at lut[lut_total + 2 * (cp_off + ...)]
template <typename PackT, typename ParamsT>
__device__ __forceinline__ void fit_packed(const PackT &pk, const double *__restrict__ lut, size_t cp_off,
                                           const ParamsT &p, float &core, float &acc, bool &failed) {
  const uint32_t cmask = (1u << p.cnt_bits) - 1u;
  const double *ef_base = lut + p.lut_total + 2 * cp_off;
  double pe = 1.0, pf = 1.0;
  for (int k = 0; k < p.nk; ++k) {
    const uint32_t c = pack_get(pk, k, p.cnt_bits, cmask, p.nk);
    const double *ef = ef_base + 2 * ((size_t)k * p.lut_kstride + c);
    if (k == 0) {
      pe = ef[0];
      pf = ef[1];
    } else {
      pe *= ef[0];
      pf *= ef[1];
    }
  }
  if (pe == pe && p.nk >= 2) {      // not NaN: every k usable
    fit_finish(pe, pf, core, acc);
    failed = false;
    return;
  }
  fit_general(pk, lut + cp_off, p, core, acc, failed);
}

// The fast path for NR of the refs a lane holds against one query (v2 epilogue): all NR x nk
// 16-byte (E, F) gathers are issued before the first is consumed -- the table look-ups are the only
// memory latency in the epilogue -- as uniform base + 32-bit lane offset (the saddr form of
// global_load).  NK > 0: straight-line code for a compile-time number of k (the default k list has
// 5); NK == 0: any nk.  Returns false -- nothing written -- when some lane of the wavefront has an
// unusable k (a NaN product), and the caller takes fit_packed pair by pair.
typedef double f64x2 __attribute__((ext_vector_type(2)));
// issue the NR x NK gathers of one batch
template <typename PackT, int NR, int NK, typename ParamsT>
__device__ __forceinline__ void ef_gather(const PackT (&pk)[NR], const double *__restrict__ lut,
                                          const uint32_t (&loff)[NR], const ParamsT &p,
                                          f64x2 (&ef)[NR][NK]) {
  const uint32_t cmask = (1u << p.cnt_bits) - 1u;
  const uint32_t kstride = (uint32_t)p.lut_kstride;
  const char *base = reinterpret_cast<const char *>(lut + p.lut_total);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const uint32_t c = pack_get(pk[r], k, p.cnt_bits, cmask, p.nk);
      const uint32_t boff = (loff[r] + (uint32_t)k * kstride + c) * 16u;
      ef[r][k] = *reinterpret_cast<const f64x2 *>(base + boff);
    }
  }
}
// products in k order; false (nothing written) when some lane of the wavefront has a NaN product
template <int NR, int NK>
__device__ __forceinline__ bool ef_finish(const f64x2 (&ef)[NR][NK], float (&core)[NR], float (&acc)[NR]) {
  double pe[NR], pf[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    pe[r] = ef[r][0].x;
    pf[r] = ef[r][0].y;
  }
#pragma unroll
  for (int k = 1; k < NK; ++k) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      pe[r] *= ef[r][k].x;
      pf[r] *= ef[r][k].y;
    }
  }
  bool all_ok = true;
#pragma unroll
  for (int r = 0; r < NR; ++r) all_ok = all_ok && (pe[r] == pe[r]);
  if (!__all(all_ok)) return false;
#pragma unroll
  for (int r = 0; r < NR; ++r) fit_finish(pe[r], pf[r], core[r], acc[r]);
  return true;
}

// any nk: running products (no gather batch to keep in registers)
struct PackWide;
struct PackParts;
template <typename PackT, int NR, typename ParamsT>
__device__ __forceinline__ std::enable_if_t<!std::is_same<PackT, PackWide>::value && !std::is_same<PackT, PackParts>::value, bool>
fit_rows_fast_anyk(const PackT (&pk)[NR], const double *__restrict__ lut, const uint32_t (&loff)[NR],
                   const ParamsT &p, float (&core)[NR], float (&acc)[NR]) {
  const uint32_t cmask = (1u << p.cnt_bits) - 1u;
  const uint32_t kstride = (uint32_t)p.lut_kstride;
  const char *base = reinterpret_cast<const char *>(lut + p.lut_total);
  double pe[NR], pf[NR];
  for (int k = 0; k < p.nk; ++k) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const uint32_t c = pack_get(pk[r], k, p.cnt_bits, cmask, p.nk);
      const uint32_t boff = (loff[r] + (uint32_t)k * kstride + c) * 16u;
      const f64x2 v = *reinterpret_cast<const f64x2 *>(base + boff);
      pe[r] = k == 0 ? v.x : pe[r] * v.x;
      pf[r] = k == 0 ? v.y : pf[r] * v.y;
    }
  }
  bool all_ok = p.nk >= 2;
#pragma unroll
  for (int r = 0; r < NR; ++r) all_ok = all_ok && (pe[r] == pe[r]);
  if (!__all(all_ok)) return false;
#pragma unroll
  for (int r = 0; r < NR; ++r) fit_finish(pe[r], pf[r], core[r], acc[r]);
  return true;
}

// ---- wide k-mer sets: nk * cnt_bits > 128 ------------------------------------------------------
// PopPUNK's default sketch size (9 984 bins, 14-bit counts) fits 9 k-mer lengths in the tile kernel's
// 128-bit count register; the documented wider lists (k = 6..15 step 1, 13..31 step 2:
// docs/sketching.rst:123-139,152-156; any np.arange(min_k, max_k + 1, k_step), PopPUNK/__main__.py:299) do not.
// The WIDE instantiation keeps the same 4x4 register tile and instruction stream and treats the register as
// a window over the k list: every wide_kpg = 128 / cnt_bits k-mer lengths a lane parks its 16 registers in
// the workgroup's SPILL SLOT -- 128 KB per group, [group][pair * 4 + dword][thread] uint32, so every store of
// a wavefront covers 256 consecutive bytes -- and starts the next group from zero; the last group follows
// after the loop and the epilogue reads every count back from the slot (each lane only ever reads what it
// wrote).  A slot belongs to a RESIDENT workgroup, not to a tile: 1 024 of them (twice what the device can
// hold) are handed out through a bitmap at the start of a workgroup and given back at its end, so the pool
// is a few hundred MB whatever the job size -- a 100 000-genome band has millions of tiles.  A slot's next
// owner may run on another XCD (another L2): every access to a slot is an agent-scope atomic (written
// through / served coherently, as in the k-split hand-over below), and the pool is touched once per
// wide_kpg * s64 compare blocks, i.e. never on the critical path.
// The fit takes the counts in k order with the same expressions as fit_packed / fit_general: a job forced
// through this path (option "wide_kpg") returns the bits the register path returns.
struct PackWide {
  const uint32_t *src;      // the lane's first dword of the pair, group 0
};
constexpr size_t WIDE_GROUP_U64 = 32 * 512;      // uint64 per (slot, group): 16 pairs x 2 x 512 threads

__device__ __forceinline__ PackW<4> wide_load(const PackWide &pk, int g) {
  const uint32_t *s = pk.src + (size_t)g * (2 * WIDE_GROUP_U64);
  PackW<4> v;
#pragma unroll
  for (int i = 0; i < 4; ++i) v.w[i] = __hip_atomic_load(s + i * 512, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}

// One scan in k order does what the register path does in two: it gathers log J for each k, accumulates the
// least-squares sums while the fit is open and notes whether EVERY k was usable.  Only then (a related pair) are
// the (E, F) products worth a second pass -- their bits are what the fast path returns; a pair with an unusable k
// finishes from the sums, which are the general statement's, and in the default (truncating) mode the scan stops at
// the first unusable k: an unrelated pair costs one or two gathers, not three passes over the list.  Same
// expressions on the same values as fit_packed / fit_general of the register path, so the same bits.
template <typename ParamsT>
__device__ __forceinline__ void fit_packed(const PackWide &pk, const double *__restrict__ lut, size_t cp_off,
                                           const ParamsT &p, float &core, float &acc, bool &failed) {
  const uint32_t cmask = (1u << p.cnt_bits) - 1u;
  const double *lutp = lut + cp_off;
  double sx = 0.0, sxx = 0.0, sy = 0.0, sxy = 0.0;
  int n = 0, k = 0;
  bool open = true, all = true;
  for (int g = 0; k < p.nk && (p.ext_skip || open); ++g) {
    const int m = p.nk - k < p.wide_kpg ? p.nk - k : p.wide_kpg;
    const PackW<4> v = wide_load(pk, g);
    for (int i = 0; i < m && (p.ext_skip || open); ++i, ++k) {
      const uint32_t c = pack_get(v, i, p.cnt_bits, cmask, m);
      const double y = lutp[(size_t)k * p.lut_kstride + c];
      const bool usable = !(y > 0.0);      // (NaN stays in: see the register version)
      all = all && usable;
      open = (p.ext_skip || open) && usable;
      if (open) {
        const double x = (double)p.kmers[k];
        sx += x;
        sxx += x * x;
        sy += y;
        sxy = __builtin_fma(x, y, sxy);
        ++n;
      }
    }
  }
  if (all && p.nk >= 2) {      // (every k usable: the scan ran to the end and the sums are complete)
    const double *ef_base = lut + p.lut_total + 2 * cp_off;
    double pe = 1.0, pf = 1.0;
    int kk = 0;
    for (int g = 0; kk < p.nk; ++g) {
      const int m = p.nk - kk < p.wide_kpg ? p.nk - kk : p.wide_kpg;
      const PackW<4> v = wide_load(pk, g);
      for (int i = 0; i < m; ++i, ++kk) {
        const uint32_t c = pack_get(v, i, p.cnt_bits, cmask, m);
        const double *ef = ef_base + 2 * ((size_t)kk * p.lut_kstride + c);
        pe = kk == 0 ? ef[0] : pe * ef[0];
        pf = kk == 0 ? ef[1] : pf * ef[1];
      }
    }
    if (pe == pe) {
      fit_finish(pe, pf, core, acc);
      failed = false;
      return;
    }
  }
  if (n < 2) {
    core = 0.0f;
    acc = 0.0f;
    failed = true;
    return;
  }
  const double dn = (double)n;
  const double slope = (dn * sxy - sx * sy) / (dn * sxx - sx * sx);
  const double icpt = (sy - slope * sx) / dn;
  core = slope < 0.0 ? (float)(1.0 - exp_nonpos(slope)) : 0.0f;
  acc = icpt < 0.0 ? (float)(1.0 - exp_nonpos(icpt)) : 0.0f;
  failed = false;
}

template <typename PackT, int NR, typename ParamsT>
__device__ __forceinline__ std::enable_if_t<std::is_same<PackT, PackWide>::value, bool>
fit_rows_fast_anyk(const PackWide (&pk)[NR], const double *__restrict__ lut, const uint32_t (&loff)[NR],
                   const ParamsT &p, float (&core)[NR], float (&acc)[NR]) {
  const uint32_t cmask = (1u << p.cnt_bits) - 1u;
  const uint32_t kstride = (uint32_t)p.lut_kstride;
  const char *base = reinterpret_cast<const char *>(lut + p.lut_total);
  double pe[NR], pf[NR];
  int k = 0;
  for (int g = 0; k < p.nk; ++g) {
    const int m = p.nk - k < p.wide_kpg ? p.nk - k : p.wide_kpg;
    PackW<4> v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] = wide_load(pk[r], g);
    for (int i = 0; i < m; ++i, ++k) {
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const uint32_t c = pack_get(v[r], i, p.cnt_bits, cmask, m);
        const uint32_t boff = (loff[r] + (uint32_t)k * kstride + c) * 16u;
        const f64x2 e = *reinterpret_cast<const f64x2 *>(base + boff);
        pe[r] = k == 0 ? e.x : pe[r] * e.x;
        pf[r] = k == 0 ? e.y : pf[r] * e.y;
      }
      // a NaN factor stays NaN: the batch cannot take the fast path any more (most tiles hold an unrelated pair
      // whose first k is already unusable -- there is no point in gathering the rest of the list for all of them)
      bool nan = false;
#pragma unroll
      for (int r = 0; r < NR; ++r) nan = nan || (pe[r] != pe[r]);
      if (__any(nan)) return false;
    }
  }
  if (p.nk < 2) return false;
#pragma unroll
  for (int r = 0; r < NR; ++r) fit_finish(pe[r], pf[r], core[r], acc[r]);
  return true;
}

// ---- k-split jobs, fit straight from the units' partial counts --------------------------------------------
// The units of a k-split tile leave their counts as 16-bit fields: uint64 [unit][query 0..3][512 threads], field r =
// the lane's ref r (dist_kernel_v2, KS_FUSED).  The tile's last unit normally rebuilds the count registers from
// them; with a wide k list there is no register to rebuild, and it fits every pair from the fields as they lie --
// count k = the sum of the k's `slices` units -- in k order with the expressions of fit_packed / fit_general.
struct PackParts {
  const unsigned long long *src;      // the lane's uint64 of (unit 0, the pair's query)
  int shift;                          // 16 * (the pair's ref within the lane)
};
constexpr size_t KS_UNIT_U64 = 4 * 512;      // uint64 per (tile, unit)
template <typename ParamsT>
__device__ __forceinline__ unsigned long long parts_word(const PackParts &pk, int k, const ParamsT &p) {
  // (fields of the k's pieces add without carrying into their neighbours: a k has at most 64 * s64 < 2^16 bins)
  unsigned long long w = 0;
  for (int h = 0; h < p.k_split; ++h)
    w += __hip_atomic_load(pk.src + (size_t)(k * p.k_split + h) * KS_UNIT_U64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return w;
}
// (one scan, then the products only for a pair whose every k is usable: see fit_packed(PackWide))
template <typename ParamsT>
__device__ __forceinline__ void fit_packed(const PackParts &pk, const double *__restrict__ lut, size_t cp_off,
                                           const ParamsT &p, float &core, float &acc, bool &failed) {
  const double *lutp = lut + cp_off;
  double sx = 0.0, sxx = 0.0, sy = 0.0, sxy = 0.0;
  int n = 0;
  bool open = true, all = true;
  for (int k = 0; k < p.nk && (p.ext_skip || open); ++k) {
    const uint32_t c = (uint32_t)(parts_word(pk, k, p) >> pk.shift) & 0xffffu;
    const double y = lutp[(size_t)k * p.lut_kstride + c];
    const bool usable = !(y > 0.0);
    all = all && usable;
    open = (p.ext_skip || open) && usable;
    if (open) {
      const double x = (double)p.kmers[k];
      sx += x;
      sxx += x * x;
      sy += y;
      sxy = __builtin_fma(x, y, sxy);
      ++n;
    }
  }
  if (all && p.nk >= 2) {
    const double *ef_base = lut + p.lut_total + 2 * cp_off;
    double pe = 1.0, pf = 1.0;
    for (int k = 0; k < p.nk; ++k) {
      const uint32_t c = (uint32_t)(parts_word(pk, k, p) >> pk.shift) & 0xffffu;
      const double *ef = ef_base + 2 * ((size_t)k * p.lut_kstride + c);
      pe = k == 0 ? ef[0] : pe * ef[0];
      pf = k == 0 ? ef[1] : pf * ef[1];
    }
    if (pe == pe) {
      fit_finish(pe, pf, core, acc);
      failed = false;
      return;
    }
  }
  if (n < 2) {
    core = 0.0f;
    acc = 0.0f;
    failed = true;
    return;
  }
  const double dn = (double)n;
  const double slope = (dn * sxy - sx * sy) / (dn * sxx - sx * sx);
  const double icpt = (sy - slope * sx) / dn;
  core = slope < 0.0 ? (float)(1.0 - exp_nonpos(slope)) : 0.0f;
  acc = icpt < 0.0 ? (float)(1.0 - exp_nonpos(icpt)) : 0.0f;
  failed = false;
}
// the NR refs of a batch share their query, i.e. their words: one load per (k, piece) serves all of them
template <typename PackT, int NR, typename ParamsT>
__device__ __forceinline__ std::enable_if_t<std::is_same<PackT, PackParts>::value, bool>
fit_rows_fast_anyk(const PackParts (&pk)[NR], const double *__restrict__ lut, const uint32_t (&loff)[NR],
                   const ParamsT &p, float (&core)[NR], float (&acc)[NR]) {
  const uint32_t kstride = (uint32_t)p.lut_kstride;
  const char *base = reinterpret_cast<const char *>(lut + p.lut_total);
  double pe[NR], pf[NR];
  for (int k = 0; k < p.nk; ++k) {
    const unsigned long long w = parts_word(pk[0], k, p);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const uint32_t c = (uint32_t)(w >> pk[r].shift) & 0xffffu;
      const uint32_t boff = (loff[r] + (uint32_t)k * kstride + c) * 16u;
      const f64x2 e = *reinterpret_cast<const f64x2 *>(base + boff);
      pe[r] = k == 0 ? e.x : pe[r] * e.x;
      pf[r] = k == 0 ? e.y : pf[r] * e.y;
    }
    // (a NaN factor stays NaN: no fast path for this batch any more -- see the PackWide form)
    bool nan = false;
#pragma unroll
    for (int r = 0; r < NR; ++r) nan = nan || (pe[r] != pe[r]);
    if (__any(nan)) return false;
  }
  if (p.nk < 2) return false;
#pragma unroll
  for (int r = 0; r < NR; ++r) fit_finish(pe[r], pf[r], core[r], acc[r]);
  return true;
}

template <int TQ, int NW, int MODE, typename PackT>
__global__ void __launch_bounds__(NW * 64)
dist_kernel(const uint64_t *__restrict__ refT, const uint32_t *__restrict__ qryT,
            const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
            const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
            void *__restrict__ out, unsigned long long *__restrict__ n_failed,
            uint64_t *__restrict__ mask_out, const DistParams p) {
  constexpr int QT = TQ * NW;                 // queries per workgroup tile
  __shared__ u32x2 lds[64 * 64];              // up to 64 bit-planes x 64 refs

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t rt = blockIdx.x;
  const size_t r = rt * 64 + lane;
  const size_t q0 = (p.q_tile0 + blockIdx.y) * QT;
  const size_t qw0 = q0 + (size_t)wave * TQ;
  // self mode: a tile entirely on or below the diagonal holds no pair (r > q needed)
  if (p.self && rt * 64 + 63 <= q0) return;
  const bool wave_active = !(p.self && rt * 64 + 63 <= qw0) && qw0 < p.q_end && qw0 + TQ > p.q_begin;

  const int bbits = p.bbits;
  const int words = p.s64 * bbits;

  uint32_t cnt[TQ];
  PackT packed[TQ];
#pragma unroll
  for (int j = 0; j < TQ; ++j) {
    cnt[j] = 0;
    pack_zero(packed[j]);
  }

  for (int k = 0; k < p.nk; ++k) {
    for (int c = 0; c < p.s64; ++c) {
      __syncthreads();  // every wave is done reading the previous block
      const size_t grow0 = (size_t)k * words + (size_t)c * bbits;
      for (int row = wave; row < bbits; row += NW) {
        const uint64_t v = refT[(grow0 + row) * p.npad_r + r];
        u32x2 t;
        t.x = (uint32_t)v;
        t.y = (uint32_t)(v >> 32);
        lds[row * 64 + lane] = t;
      }
      __syncthreads();
      if (wave_active) {
        // wave-uniform query words for this 64-bin block: SGPR operands
        const uint32_t *__restrict__ qp = qryT + 2 * (grow0 * p.npad_q + qw0);
        const u32x2 *lrow = lds + lane;
        uint32_t lo[TQ], hi[TQ];
#pragma unroll
        for (int j = 0; j < TQ; ++j) {
          lo[j] = 0xffffffffu;
          hi[j] = 0xffffffffu;
        }
        for (int b = 0; b < bbits; ++b) {
          const u32x2 a = lrow[b * 64];
          const uint32_t *qb = qp + (size_t)b * 2 * p.npad_q;
#pragma unroll
          for (int j = 0; j < TQ; ++j) {
            lo[j] = __builtin_amdgcn_bitop3_b32(lo[j], a.x, qb[2 * j], 0x90);
            hi[j] = __builtin_amdgcn_bitop3_b32(hi[j], a.y, qb[2 * j + 1], 0x90);
          }
        }
#pragma unroll
        for (int j = 0; j < TQ; ++j) cnt[j] += __popc(lo[j]) + __popc(hi[j]);
      }
    }
    // ---- end of one k: consume the counts --------------------------------
    if (wave_active) {
#pragma unroll
      for (int j = 0; j < TQ; ++j) {
        if constexpr (MODE == MODE_DIST || ppk_is_mask(MODE)) {
          pack_put(packed[j], cnt[j], k, p.cnt_bits);
        } else {
          const size_t q = qw0 + j;
          const bool valid = r < p.n_ref && q >= p.q_begin && q < p.q_end && (!p.self || r > q);
          if (valid) {
            const size_t row = (p.self ? q * p.n_ref - (q * (q + 1)) / 2 + (r - q - 1)
                                       : q * p.n_ref + r) - p.row_base;
            if constexpr (MODE == MODE_COUNTS) {
              static_cast<uint32_t *>(out)[row * p.nk + k] = cnt[j];
            } else {
              double jr = 0.0;
              if (p.random_correct) {
                const int cr = ref_clu ? ref_clu[r] : 0;
                const int cq = qry_clu ? qry_clu[q] : 0;
                jr = (double)rtab[((size_t)k * p.n_clu + cr) * p.n_clu + cq];
              }
              static_cast<float *>(out)[row * p.nk + k] =
                  (float)observed_excess(jaccard_obs(cnt[j], p.s64, bbits, p.ext_adjust), jr);
            }
          }
        }
        cnt[j] = 0;
      }
    }
  }

  // ---- epilogue: regression (+ boundary) per pair ---------------------------
  if constexpr (MODE == MODE_DIST || ppk_is_mask(MODE)) {
    if (!wave_active) return;
    const int cr = (ref_clu && r < p.n_ref) ? ref_clu[r] : 0;
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      const size_t q = qw0 + j;   // wave-uniform
      if (q < p.q_begin || q >= p.q_end) continue;
      const bool valid = r < p.n_ref && (!p.self || r > q);
      const int cq = qry_clu ? qry_clu[q] : 0;
      const size_t cp_off = (size_t)(cr * p.n_clu + cq) * p.lut_cpstride;
      float core = 0.0f, acc = 0.0f;
      bool failed = false;
      if (valid) fit_packed<PackT>(packed[j], lut, cp_off, p, core, acc, failed);
      if (n_failed) {
        const uint64_t fm = __ballot(valid && failed);
        if (fm && lane == 0) atomicAdd(n_failed, (unsigned long long)__popcll(fm));
      }
      if constexpr (MODE == MODE_DIST) {
        if (valid) {
          const size_t row = (p.self ? q * p.n_ref - (q * (q + 1)) / 2 + (r - q - 1)
                                     : q * p.n_ref + r) - p.row_base;
          float2 v;
          v.x = core;
          v.y = acc;
          static_cast<float2 *>(out)[row] = v;
        }
      } else {
        bool pred = false;
        if (valid) {
          if constexpr (MODE == MODE_BGMM) {
            const ppk_bgmm &bg = *static_cast<const ppk_bgmm *>(out);
            pred = ppk_bgmm_label(core, acc, bg) == bg.within_label;
          } else {
            // RefineFit.assign pre-scales X/scale in float32 (PopPUNK/models.py:1085-1089)
            const float xs = __fdiv_rn(core, p.scale_x), ys = __fdiv_rn(acc, p.scale_y);
            const float s = ppk_line_dist(xs, ys, p.x_max, p.y_max, p.slope);
            pred = p.inclusive ? (s <= 0.0f) : (s < 0.0f);
          }
        }
        const uint64_t m = __ballot(pred);
        if (lane == 0) mask_out[(q - p.q_begin) * p.n_rtiles + rt] = m;
      }
    }
  }
}


// ---- v2: 256 x 32 pair tile, LDS-DMA double buffer, 4x4 register tile ----------------------

#define PPK_GPTR(p) ((const __attribute__((address_space(1))) void *)(p))
#define PPK_LPTR(p) ((__attribute__((address_space(3))) void *)(p))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int V2_R = 4, V2_TQ = 4, V2_RT = 256, V2_BB = 14;
static_assert(RANK_BB == V2_BB, "rank codes are built for the tile kernels' bbits");
// byte offset of `DistParams p` in dist_kernel_v2's kernarg segment: nine 8-byte pointers precede it
constexpr int V2_PARAMS_KERNARG_OFFSET = 9 * 8;

// Non-empty tiles of ref tiles 0 .. r-1, in ref-tile-major order.  Rectangle: every ref tile pairs
// with all q_tiles query tiles.  Triangle (self): ref tile i has a pair with r > q only for the
// first clamp(m*i + c0, 0, q_tiles) query tiles (m = 256 / queries-per-tile).
inline unsigned long long tiles_before64(unsigned r, int self, unsigned q_tiles, int m, int c0) {
  if (!self) return (unsigned long long)r * q_tiles;
  // i_lo: first ref tile with any query tile; i_hi: first with all of them
  const long long i_lo = c0 > 0 ? 0 : (-c0) / m + 1;
  long long i_hi = ((long long)q_tiles - c0 + m - 1) / m;
  if (i_hi < i_lo) i_hi = i_lo;
  const long long rr = (long long)r;
  const long long b = rr < i_hi ? rr : i_hi;
  unsigned long long t = 0;
  if (b > i_lo) t = (unsigned long long)((m * (b * (b - 1) - i_lo * (i_lo - 1))) / 2 + c0 * (b - i_lo));
  if (rr > i_hi) t += (unsigned long long)(rr - i_hi) * q_tiles;
  return t;
}
// The device copy stays in 32-bit arithmetic: the launcher has checked (with the 64-bit version)
// that every count fits, and 64-bit scalars in the tile decode cost the tile kernels registers
// they do not have (VGPR spills 6 -> 14, -3 %).
__device__ __forceinline__ unsigned tiles_before(unsigned r, int self, unsigned q_tiles, int m, int c0) {
  if (!self) return r * q_tiles;
  const int i_lo = c0 > 0 ? 0 : (-c0) / m + 1;
  int i_hi = ((int)q_tiles - c0 + m - 1) / m;
  if (i_hi < i_lo) i_hi = i_lo;
  const int rr = (int)r;
  const int b = rr < i_hi ? rr : i_hi;
  unsigned t = 0;
  if (b > i_lo) t = (unsigned)((m * (b * (b - 1) - i_lo * (i_lo - 1))) / 2 + c0 * (b - i_lo));
  if (rr > i_hi) t += (unsigned)(rr - i_hi) * q_tiles;
  return t;
}

// MODE_MASK_ROWS / MODE_BGMM_ROWS: the rows of one query's four mask words, staged.  ball[0] / ball[1] are the
// predicate of the even / odd refs of r0 .. r0+127, ball[2] / ball[3] of r0+128 .. r0+255, and lane l holds refs 2l and
// 2l+1 of each half: lane order, even before odd, is bit order across a half's two consecutive mask words.  One lane
// reserves the wavefront's rows of this query with ONE atomicAdd (nothing when no bit is set); the position of a word's
// first row goes to rows_base, parallel to the mask, for the words that exist and have a bit; a lane stores its rows at
// the reservation + the bits before its own, when that lies inside the staging buffer.  Which reservation a wavefront
// gets depends on timing; what the expand pass (mask_expand_kernel<SCAN, true>) copies out of it, by rows_base, does not.
// word0: the first of the four words' index in the band's mask; n_words: how many of the four the mask has.
template <typename ParamsT>
__device__ __forceinline__ void rows_emit(const uint64_t (&ball)[4], const float (&core)[4], const float (&acc)[4], int lane,
                                          size_t word0, size_t n_words, const ParamsT &p) {
  const unsigned c0 = (unsigned)__popcll(ball[0]) + (unsigned)__popcll(ball[1]);
  const unsigned c1 = (unsigned)__popcll(ball[2]) + (unsigned)__popcll(ball[3]);
  if (c0 + c1 == 0) return;      // wave-uniform
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(p.rows_count, (unsigned long long)(c0 + c1));
  base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  if (lane == 0) {
    // words 2h / 2h+1 hold lanes 0..31 / 32..63 of half h
    const unsigned lo0 = (unsigned)__popc((uint32_t)ball[0]) + (unsigned)__popc((uint32_t)ball[1]);
    const unsigned lo1 = (unsigned)__popc((uint32_t)ball[2]) + (unsigned)__popc((uint32_t)ball[3]);
    unsigned long long *wb = p.rows_base + word0;
    if (n_words > 0 && lo0) wb[0] = base;
    if (n_words > 1 && c0 != lo0) wb[1] = base + lo0;
    if (n_words > 2 && lo1) wb[2] = base + c0;
    if (n_words > 3 && c1 != lo1) wb[3] = base + c0 + lo1;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t e = ball[2 * h], o = ball[2 * h + 1];
    const unsigned below =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(e >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)e, 0u)) +
        __builtin_amdgcn_mbcnt_hi((uint32_t)(o >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)o, 0u));
    const bool pe = (e >> lane) & 1, po = (o >> lane) & 1;
    const unsigned long long pos = base + (h ? c0 : 0u) + below;
    if (pe && pos < p.rows_cap) p.rows_stage[pos] = make_float2(core[2 * h], acc[2 * h]);
    if (po && pos + (pe ? 1u : 0u) < p.rows_cap) p.rows_stage[pos + (pe ? 1u : 0u)] = make_float2(core[2 * h + 1], acc[2 * h + 1]);
  }
}

// NW = wavefronts per workgroup: 8 (256 x 32 tile, 2 workgroups per CU).  The 16-wavefront shape
// (256 x 64 tile, one workgroup per CU) was measured and rejected (tools/ubench_pipe.hip).
// W = dwords of the per-pair count register (1 in the COUNTS / JACCARD modes, which consume each
// k's counts at once)
// WIDE: the count register is a window over the k list (PackWide above).  EXP: the experiments build's
// instantiation -- `ablate` and the rejected tile orders exist only there, so the product kernel carries neither
// their tests nor a live scalar for them.
template <int NW, int MODE, int W, bool KSPLIT = false, bool WIDE = false, bool EXP = false>
__global__ void __launch_bounds__(NW * 64, 4)
dist_kernel_v2(const uint64_t *__restrict__ refT, const uint64_t *__restrict__ qryT,
               const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
               const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
               void *__restrict__ out, unsigned long long *__restrict__ n_failed,
               uint64_t *__restrict__ mask_out, const DistParams p) {
  constexpr int PL = V2_BB;      // raw planes
  constexpr bool FOLD2 = false, FOLDH = false;
#include "ppk_dist_tile.inc"
}

// The whole-tile kernel of the two-dword count register on a rank-coded database: refT / qryT are the injective copy (PpkCoding),
// [k][block * PL + plane][npad].  Same arguments at the same kernarg offsets (the epilogue reads DistParams there).
template <int PL, int MODE>
__global__ void __launch_bounds__(8 * 64, 4)
dist_kernel_v2_rank(const uint64_t *__restrict__ refT, const uint64_t *__restrict__ qryT,
                    const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
                    const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
                    void *__restrict__ out, unsigned long long *__restrict__ n_failed,
                    uint64_t *__restrict__ mask_out, const DistParams p) {
  constexpr int NW = 8, W = 2;
  constexpr bool KSPLIT = false, WIDE = false, EXP = false, FOLD2 = false, FOLDH = false;
#include "ppk_dist_tile.inc"
}

// The same kernel at 8 planes on the two-holder pair (PPK_CODING_FOLD2): FOLD2 compiles one more block into
// the body, at the top of the epilogue, which adds the tile's events (DistParams::fold2_ev) to the counts.  A kernel of
// its own name: dist_kernel_v2_rank<PL, MODE> stays the code (and the symbols) it was.
template <int MODE>
__global__ void __launch_bounds__(8 * 64, 4)
dist_kernel_v2_fold2(const uint64_t *__restrict__ refT, const uint64_t *__restrict__ qryT,
                     const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
                     const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
                     void *__restrict__ out, unsigned long long *__restrict__ n_failed,
                     uint64_t *__restrict__ mask_out, const DistParams p) {
  constexpr int NW = 8, W = 2, PL = 8;
  constexpr bool KSPLIT = false, WIDE = false, EXP = false, FOLD2 = true, FOLDH = false;
#include "ppk_dist_tile.inc"
}

// The same kernel on the holder pair (PPK_CODING_FOLDH: the 8-plane coding, stored and copied as a 4-plane chunk,
// PPK_FOLDH_CHUNK_PLANES -- planes 4 .. 7 are zero in every block, so a block is 8 ref pieces and one query piece, 9 KB
// through L2 into LDS instead of 18, two DMA pieces per wavefront instead of three).
// FOLDH swaps the three streams for the 4- / 3- / 2-plane ones and the correction block for the one that adds the
// database's 12-bit entries (DistParams::fold2_ev / fold2_off carry its d_list / d_off; rank_short / fold2_six
// the 3- and the 2-plane flags).  A kernel of its own name again: every other symbol stays the code it was.
template <int MODE>
__global__ void __launch_bounds__(8 * 64, 4)
dist_kernel_v2_foldh(const uint64_t *__restrict__ refT, const uint64_t *__restrict__ qryT,
                     const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
                     const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
                     void *__restrict__ out, unsigned long long *__restrict__ n_failed,
                     uint64_t *__restrict__ mask_out, const DistParams p) {
  constexpr int NW = 8, W = 2, PL = 8;
  constexpr bool KSPLIT = false, WIDE = false, EXP = false, FOLD2 = true, FOLDH = true;
#include "ppk_dist_tile.inc"
}

// The coded kernels in the rows modes (MODE_MASK_ROWS / MODE_BGMM_ROWS), under names of their own once more: the rank,
// fold2 and foldh kernels keep exactly the instantiations (and symbols) they had.
template <int PL, int MODE>
__global__ void __launch_bounds__(8 * 64, 4)
dist_kernel_v2_rank_rows(const uint64_t *__restrict__ refT, const uint64_t *__restrict__ qryT,
                         const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
                         const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
                         void *__restrict__ out, unsigned long long *__restrict__ n_failed,
                         uint64_t *__restrict__ mask_out, const DistParams p) {
  static_assert(ppk_is_rows(MODE), "rows modes");
  constexpr int NW = 8, W = 2;
  constexpr bool KSPLIT = false, WIDE = false, EXP = false, FOLD2 = false, FOLDH = false;
#include "ppk_dist_tile.inc"
}
template <int MODE, bool HOLDERS>
__global__ void __launch_bounds__(8 * 64, 4)
dist_kernel_v2_fold_rows(const uint64_t *__restrict__ refT, const uint64_t *__restrict__ qryT,
                         const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
                         const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab,
                         void *__restrict__ out, unsigned long long *__restrict__ n_failed,
                         uint64_t *__restrict__ mask_out, const DistParams p) {
  static_assert(ppk_is_rows(MODE), "rows modes");
  constexpr int NW = 8, W = 2, PL = 8;
  constexpr bool KSPLIT = false, WIDE = false, EXP = false, FOLD2 = true, FOLDH = HOLDERS;
#include "ppk_dist_tile.inc"
}


// ---- generic fallback: counts -> distances when nk * count-bits does not fit 128 bits ---------
// (e.g. 17 k-mer lengths at s = 10 000).  dist_kernel* write the raw counts, this kernel does
// a4-a6 per row with the expression order of the CPU statement.
// (q, r) of distance row `row` of a job: the "query" and the "ref" sample (ppk.h: self: row <-> (q < r), condensed)
__device__ __forceinline__ void row_samples(size_t row, int self, size_t n_ref, size_t &q, size_t &r) {
  if (self) {
    // condensed row -> (q, r): largest q with q*n - q(q+1)/2 <= row
    const double d = sqrt((double)(4 * n_ref * (n_ref - 1)) - 8.0 * (double)row - 7.0);
    long long qi = (long long)n_ref - 2 - (long long)floor(d / 2.0 - 0.5);
    if (qi < 0) qi = 0;
    while (qi > 0 && (size_t)qi * n_ref - ((size_t)qi * ((size_t)qi + 1)) / 2 > row) --qi;
    while ((size_t)(qi + 1) * n_ref - ((size_t)(qi + 1) * ((size_t)qi + 2)) / 2 <= row) ++qi;
    q = (size_t)qi;
    r = row - (q * n_ref - (q * (q + 1)) / 2) + q + 1;
  } else {
    q = row / n_ref;
    r = row % n_ref;
  }
}

// One row of the generic regression: `cnt` its nk counts (cnt[k * k_stride]), (q, r) its samples (read only with a
// multi-cluster table).  The dense route names the row by its index, the pair-list route by its samples.
__device__ __forceinline__ bool regress_counts_row(const uint32_t *__restrict__ cnt, size_t k_stride, size_t q, size_t r,
                                                   int nk, const int *__restrict__ kmers, size_t s64, size_t bbits,
                                                   const float *__restrict__ rtab, int n_clu,
                                                   const uint16_t *__restrict__ ref_clu,
                                                   const uint16_t *__restrict__ qry_clu, float scale_x, float scale_y,
                                                   int ext_adjust, int ext_skip, float2 &v) {
  bool failed = false;
  const double tol = 5.0 / (double)(s64 * 64);
  double sx = 0.0, sxx = 0.0, sy = 0.0, sxy = 0.0;
  int n = 0;
  bool open = true;
  for (int k = 0; k < nk; ++k) {
    double jr = 0.0;
    if (rtab) {
      const int cr = (n_clu > 1 && ref_clu) ? ref_clu[r] : 0;
      const int cq = (n_clu > 1 && qry_clu) ? qry_clu[q] : 0;
      jr = (double)rtab[((size_t)k * n_clu + cr) * n_clu + cq];
    }
    const double j = observed_excess(jaccard_obs(cnt[(size_t)k * k_stride], s64, bbits, ext_adjust), jr);
    open = (ext_skip || open) && !(j < tol);
    if (open) {
      const double x = (double)kmers[k], y = log(j);
      sx += x;
      sxx += x * x;
      sy += y;
      sxy += x * y;
      ++n;
    }
  }
  float core = 0.0f, acc = 0.0f;
  if (n < 2) {
    failed = true;
  } else {
    const double dn = (double)n;
    const double slope = (dn * sxy - sx * sy) / (dn * sxx - sx * sx);
    const double icpt = (sy - slope * sx) / dn;
    core = slope < 0.0 ? (float)(1.0 - exp(slope)) : 0.0f;
    acc = icpt < 0.0 ? (float)(1.0 - exp(icpt)) : 0.0f;
  }
  v.x = __fdiv_rn(core, scale_x);
  v.y = __fdiv_rn(acc, scale_y);
  return failed;
}

__global__ void __launch_bounds__(256)
regress_counts_kernel(const uint32_t *__restrict__ counts, size_t n_rows, size_t row_base, int self,
                      size_t n_ref, int nk, const int *__restrict__ kmers, size_t s64, size_t bbits,
                      const float *__restrict__ rtab, int n_clu,
                      const uint16_t *__restrict__ ref_clu, const uint16_t *__restrict__ qry_clu,
                      float scale_x, float scale_y, int ext_adjust, int ext_skip,
                      float2 *__restrict__ out, unsigned long long *__restrict__ n_failed) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool failed = false;
  if (i < n_rows) {
    size_t q = 0, r = 0;
    if (rtab && n_clu > 1) row_samples(row_base + i, self, n_ref, q, r);
    float2 v;
    failed = regress_counts_row(counts + i * nk, 1, q, r, nk, kmers, s64, bbits, rtab, n_clu, ref_clu, qry_clu, scale_x,
                                scale_y, ext_adjust, ext_skip, v);
    out[i] = v;
  }
  if (n_failed) {
    const uint64_t fm = __ballot(failed);
    if (fm && (threadIdx.x & 63) == 0) atomicAdd(n_failed, (unsigned long long)__popcll(fm));
  }
}

// ---- k-split jobs: counts -> distances with the SAME fit as the tile epilogue -------------------
// The row's counts where the counts pass left them, [k * slices + piece][row]: read k by k, in the order and with the
// expressions of fit_packed / fit_general, so a k list of any length (the wide ones too) gets the bits the tile kernel
// gives.
struct PackRows {
  const uint32_t *counts;      // the row's first count
  size_t n_rows;
  int slices;
};
__device__ __forceinline__ uint32_t rows_get(const PackRows &pk, int k) {
  uint32_t c = 0;
  for (int h = 0; h < pk.slices; ++h) c += pk.counts[((size_t)k * pk.slices + h) * pk.n_rows];
  return c;
}
template <typename ParamsT>
__device__ __forceinline__ void fit_general(const PackRows &pk, const double *__restrict__ lutp, const ParamsT &p,
                                            float &core, float &acc, bool &failed) {
  double sx = 0.0, sxx = 0.0, sy = 0.0, sxy = 0.0;
  int n = 0;
  bool open = true;
  for (int k = 0; k < p.nk; ++k) {
    const double y = lutp[(size_t)k * p.lut_kstride + rows_get(pk, k)];
    open = (p.ext_skip || open) && !(y > 0.0);
    if (open) {
      const double x = (double)p.kmers[k];
      sx += x;
      sxx += x * x;
      sy += y;
      sxy = __builtin_fma(x, y, sxy);
      ++n;
    }
  }
  if (n < 2) {
    core = 0.0f;
    acc = 0.0f;
    failed = true;
    return;
  }
  const double dn = (double)n;
  const double slope = (dn * sxy - sx * sy) / (dn * sxx - sx * sx);
  const double icpt = (sy - slope * sx) / dn;
  core = slope < 0.0 ? (float)(1.0 - exp_nonpos(slope)) : 0.0f;
  acc = icpt < 0.0 ? (float)(1.0 - exp_nonpos(icpt)) : 0.0f;
  failed = false;
}
template <typename ParamsT>
__device__ __forceinline__ void fit_packed(const PackRows &pk, const double *__restrict__ lut, size_t cp_off,
                                           const ParamsT &p, float &core, float &acc, bool &failed) {
  const double *ef_base = lut + p.lut_total + 2 * cp_off;
  double pe = 1.0, pf = 1.0;
  for (int k = 0; k < p.nk; ++k) {
    const double *ef = ef_base + 2 * ((size_t)k * p.lut_kstride + rows_get(pk, k));
    pe = k == 0 ? ef[0] : pe * ef[0];
    pf = k == 0 ? ef[1] : pf * ef[1];
  }
  if (pe == pe && p.nk >= 2) {
    fit_finish(pe, pf, core, acc);
    failed = false;
    return;
  }
  fit_general(pk, lut + cp_off, p, core, acc, failed);
}

// One row of the k-split regression: its counts at counts[k * n_rows] (one piece per k unless p.k_split says more),
// (q, r) its samples, read only with a multi-cluster table (ref_clu non-null).
__device__ __forceinline__ bool regress_packed_row(const uint32_t *__restrict__ counts, size_t n_rows, int slices,
                                                   size_t q, size_t r, const double *__restrict__ lut,
                                                   const uint16_t *__restrict__ ref_clu,
                                                   const uint16_t *__restrict__ qry_clu, const DistParams &p,
                                                   float2 &v) {
  bool failed = false;
  size_t cp = 0;
  if (p.n_clu > 1 && ref_clu) cp = (size_t)ref_clu[r] * p.n_clu + (qry_clu ? qry_clu[q] : 0);
  PackRows pk;      // a k's blocks were counted in `k_split` pieces: [k * slices + piece][row]
  pk.counts = counts;
  pk.n_rows = n_rows;
  pk.slices = slices;
  float core, acc;
  fit_packed(pk, lut, cp * p.lut_cpstride, p, core, acc, failed);
  v = make_float2(core, acc);
  return failed;
}

__global__ void __launch_bounds__(256)
regress_packed_kernel(const uint32_t *__restrict__ counts, size_t n_rows, const double *__restrict__ lut,
                      const uint16_t *__restrict__ ref_clu, const uint16_t *__restrict__ qry_clu,
                      float2 *__restrict__ out, unsigned long long *__restrict__ n_failed,
                      const DistParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool failed = false;
  if (i < n_rows) {
    size_t q = 0, r = 0;
    if (p.n_clu > 1 && ref_clu) row_samples(p.row_base + i, p.self, p.n_ref, q, r);
    float2 v;
    failed = regress_packed_row(counts + i, n_rows, p.k_split, q, r, lut, ref_clu, qry_clu, p, v);
    out[i] = v;
  }
  if (n_failed) {
    const uint64_t fm = __ballot(failed);
    if (fm && (threadIdx.x & 63) == 0) atomicAdd(n_failed, (unsigned long long)__popcll(fm));
  }
}

// ---- pair lists: the rows of listed pairs, without the matrix (ppk_dist_pairs_dev) -----------------
// Per chunk of the list: the samples it names get a slot each (mark), their sketches are gathered out of
// [k][word][sample] into a row image R[slot][(k * bbits + plane) * s64 + block] by an LDS tile transpose (the
// inverse of transpose_kernel, planes outermost within a k so that the lanes of a pair read consecutive words), a
// group of lanes counts each pair's matches per k from two rows, and the row is fitted by the statements of the dense
// route (regress_packed_row, regress_counts_row, the tiles' Jaccard statement).  The counts are integers, so a pair's
// bits do not depend on the chunk, the slot or the lanes that counted it.
struct PairsGeom {
  long long n_ref, n_qry, off;      // n_qry 0: a self job
  const long long *i, *j;
  size_t stride;
};
constexpr uint32_t kNoSlot = 0xffffffffu, kSlotPending = 0xfffffffeu;

// Edge ids -> a = min - off, b = max - off, as ppk_edge_weights_dev reads them: samples a < b of a self job, ref a and
// query b - n_ref otherwise.  False for a pair that names no row of the dense result.
__device__ __forceinline__ bool pair_ends(const PairsGeom &g, size_t p, long long &a, long long &b) {
  const long long i = g.i[p * g.stride], j = g.j[p * g.stride];
  a = (i < j ? i : j) - g.off;
  b = (i < j ? j : i) - g.off;
  if (g.n_qry == 0) return a >= 0 && b < g.n_ref && a != b;
  return a >= 0 && a < g.n_ref && b >= g.n_ref && b - g.n_ref < g.n_qry;
}
// the "query" and the "ref" sample of a checked pair, in the dense route's meaning (row_samples)
__device__ __forceinline__ void pair_samples(const PairsGeom &g, long long a, long long b, size_t &q, size_t &r) {
  q = g.n_qry == 0 ? (size_t)a : (size_t)(b - g.n_ref);
  r = g.n_qry == 0 ? (size_t)b : (size_t)a;
}

// the smallest p whose pair names no row (nothing is read through an id here)
__global__ void __launch_bounds__(256) pairs_validate_kernel(const PairsGeom g, size_t n_pairs, unsigned long long *bad) {
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (size_t)gridDim.x * 256) {
    long long a, b;
    if (!pair_ends(g, p, a, b)) atomicMin(bad, (unsigned long long)p);
  }
}

// slot[u] of every sample u the chunk [p0, p0 + n) names (a self job: u = sample; otherwise refs first, query q at
// n_ref + q, which is b itself): the order of arrival, counted in slot[n_tot].  The array comes in as all-ones, so the
// counter's first value is 0 after the increment wraps.  Which slot a sample gets changes no result.
__global__ void __launch_bounds__(256)
pairs_mark_kernel(const PairsGeom g, size_t p0, size_t n, uint32_t *slot, size_t n_tot) {
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < 2 * n; t += (size_t)gridDim.x * 256) {
    long long a, b;
    pair_ends(g, p0 + (t >> 1), a, b);
    const size_t u = (size_t)((t & 1) ? b : a);
    if (atomicCAS(slot + u, kNoSlot, kSlotPending) == kNoSlot) slot[u] = atomicAdd(slot + n_tot, 1u) + 1u;
  }
}

// R[slot[s]][c'] = skT[c * npad + s] for the named samples s of one database; c' = (k * bbits + plane) * s64 + block
// is word c = k * words + block * bbits + plane.  A workgroup moves 32 words x 32 samples: 256-byte runs along the
// sample axis in, 256-byte runs along the row out; a tile of 32 samples none of which is named is skipped.
__global__ void __launch_bounds__(256)
pairs_gather_kernel(const uint64_t *__restrict__ skT, size_t n, size_t npad, const uint32_t *__restrict__ slot,
                    uint64_t *__restrict__ R, size_t cols, int s64, int bbits) {
  __shared__ uint64_t tile[32][33];
  __shared__ uint32_t sl[32];
  const size_t c0 = (size_t)blockIdx.x * 32, s0 = (size_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  uint32_t mine = kNoSlot;
  if (threadIdx.x < 32) {
    if (s0 + threadIdx.x < n) mine = slot[s0 + threadIdx.x];
    sl[threadIdx.x] = mine;
  }
  if (!__syncthreads_or(mine != kNoSlot)) return;
  const size_t words = (size_t)s64 * bbits;
  for (int i = ty; i < 32; i += 8) {
    const size_t cp = c0 + i;
    if (cp < cols) {
      const size_t k = cp / words, rem = cp % words, b = rem / s64, blk = rem % s64;
      tile[i][tx] = skT[(k * words + blk * bbits + b) * npad + s0 + tx];      // (s0 + tx < npad: a multiple of 256)
    }
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const uint32_t row = sl[i];
    if (row != kNoSlot && c0 + tx < cols) R[(size_t)row * cols + c0 + tx] = tile[tx][i];
  }
}

// Match counts of the chunk's pairs: cnt[k * k_stride + pair * p_stride].  G lanes (a power of two, at most 64) take
// one pair, lane l the 64-bin blocks l, l + G, ...: per plane bits &= ~(a ^ b) on both halves, as kernel 1, then the
// popcounts; a k's sum over the G lanes is an integer sum.  A wave works through a contiguous span of the list, 64 / G
// pairs at a time, so the rows a row-ordered list repeats stay in the cache next to it.
__global__ void __launch_bounds__(256)
pairs_counts_kernel(const uint64_t *__restrict__ R, size_t cols, const uint32_t *__restrict__ slot, const PairsGeom g,
                    size_t p0, size_t n, size_t span, int G, int nk, int s64, int bbits, uint32_t *__restrict__ cnt,
                    size_t k_stride, size_t p_stride) {
  const int lane = threadIdx.x & 63, sub = lane / G, l = lane % G;
  const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const size_t lo = wave * span < n ? wave * span : n, hi = lo + span < n ? lo + span : n;
  for (size_t base = lo; base < hi; base += (size_t)(64 / G)) {      // (wave-uniform)
    const size_t pl = base + sub;
    const bool active = pl < hi;
    const uint64_t *ra = R, *rb = R;
    if (active) {
      long long a, b;
      pair_ends(g, p0 + pl, a, b);
      ra = R + (size_t)slot[a] * cols;
      rb = R + (size_t)slot[b] * cols;
    }
    for (int k = 0; k < nk; ++k) {
      uint32_t c = 0;
      if (active)
        for (int blk = l; blk < s64; blk += G) {
          uint32_t x = 0xffffffffu, y = 0xffffffffu;
          for (int b = 0; b < bbits; ++b) {
            const size_t w = ((size_t)k * bbits + b) * s64 + blk;
            const uint64_t va = ra[w], vb = rb[w];
            x = __builtin_amdgcn_bitop3_b32(x, (uint32_t)va, (uint32_t)vb, 0x90);
            y = __builtin_amdgcn_bitop3_b32(y, (uint32_t)(va >> 32), (uint32_t)(vb >> 32), 0x90);
          }
          c += __popc(x) + __popc(y);
        }
      for (int o = G >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if (active && l == 0) cnt[(size_t)k * k_stride + pl * p_stride] = c;
    }
  }
}

// The chunk's rows from its counts, one thread per pair.  FIT 0: regress_packed_row on counts [k][pair] (the databases
// the tile kernels take); 1: regress_counts_row on counts [pair][k] (ppk_unfused); 2: the tiles' Jaccard statement on
// counts [pair][k].  `out` is the chunk's first row.
template <int FIT>
__global__ void __launch_bounds__(256)
pairs_fit_kernel(const uint32_t *__restrict__ cnt, size_t n, const PairsGeom g, size_t p0,
                 const double *__restrict__ lut, const uint16_t *__restrict__ ref_clu,
                 const uint16_t *__restrict__ qry_clu, const float *__restrict__ rtab, const int *__restrict__ kmers,
                 void *__restrict__ out, unsigned long long *__restrict__ n_failed, const DistParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool failed = false;
  if (i < n) {
    long long a, b;
    pair_ends(g, p0 + i, a, b);
    size_t q, r;
    pair_samples(g, a, b, q, r);
    if constexpr (FIT == 2) {
      for (int k = 0; k < p.nk; ++k) {
        double jr = 0.0;
        if (p.random_correct) {
          const int cr = ref_clu ? ref_clu[r] : 0;
          const int cq = qry_clu ? qry_clu[q] : 0;
          jr = (double)rtab[((size_t)k * p.n_clu + cr) * p.n_clu + cq];
        }
        static_cast<float *>(out)[i * p.nk + k] =
            (float)observed_excess(jaccard_obs(cnt[i * p.nk + k], p.s64, p.bbits, p.ext_adjust), jr);
      }
    } else {
      float2 v;
      if constexpr (FIT == 0)
        failed = regress_packed_row(cnt + i, n, 1, q, r, lut, ref_clu, qry_clu, p, v);
      else
        failed = regress_counts_row(cnt + i * p.nk, 1, q, r, p.nk, kmers, p.s64, p.bbits, rtab, p.n_clu, ref_clu, qry_clu,
                                    p.scale_x, p.scale_y, p.ext_adjust, p.ext_skip, v);
      static_cast<float2 *>(out)[i] = v;
    }
  }
  if (FIT != 2 && n_failed) {
    const uint64_t fm = __ballot(failed);
    if (fm && (threadIdx.x & 63) == 0) atomicAdd(n_failed, (unsigned long long)__popcll(fm));
  }
}

// ---- host-side launch ------------------------------------------------------

// bits of one packed count: the fewest that hold 0 .. 64 * s64
static int count_bits(size_t s64) {
  int bits = 1;
  while (((size_t)1 << bits) <= s64 * 64) ++bits;
  return bits;
}
// the options the route choice reads
static PpkRouteKnobs route_knobs() {
  const PpkConfig &c = ppk_config();
  return {c.ksplit.load(), c.ksplit_wide.load(), c.ksplit_long.load(), c.ksplit_fused.load(), c.ksplit_slices.load(),
          c.wide_kpg.load(), (size_t)c.ksplit_scratch_mb.load() << 20};
}
// distance rows of the band [p.q_begin, p.q_end) (p.row_base: the rows before it)
static size_t band_rows(const DistParams &p) {
  return p.self ? (p.q_end * p.n_ref - (p.q_end * (p.q_end + 1)) / 2) - p.row_base : (p.q_end - p.q_begin) * p.n_ref;
}

namespace {

// The pointer arguments of the pair-tile kernels, in their order (DistParams follows them)
struct DistArgs {
  const uint64_t *sk_r, *sk_q;
  const double *lut;
  const uint16_t *rclu, *qclu;      // cluster ids: only where a multi-cluster random-match table is in use
  const float *rtab;
  void *out;
  unsigned long long *n_failed;
  uint64_t *mask;
};

// One launch of a pair-tile kernel, timed under `name` while the profiler is on.  (Q: dist_kernel reads its query words
// as dwords.)
template <typename Q, typename... Tail>
int launch_kernel(void (*kernel)(const uint64_t *, const Q *, Tail...), dim3 grid, dim3 block, const char *name,
                  const DistArgs &a, const DistParams &p, hipStream_t s) {
  ppk_set_kernel_name(name);
  ppk_prof_begin(s);
  hipLaunchKernelGGL(kernel, grid, block, 0, s, a.sk_r, reinterpret_cast<const Q *>(a.sk_q), a.lut, a.rclu, a.qclu,
                     a.rtab, a.out, a.n_failed, a.mask, p);
  ppk_prof_end(s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

template <int TQ, int NW, int MODE, typename PackT>
int launch_variant(const DistArgs &a, DistParams &p, hipStream_t s, const char *name) {
  constexpr int QT = TQ * NW;
  p.q_tile0 = p.q_begin / QT;
  const size_t q_tiles = (p.q_end + QT - 1) / QT - p.q_tile0;
  if (q_tiles == 0 || p.n_rtiles == 0) return PPK_OK;
  if (q_tiles > 65535) return ppk_fail(PPK_ERR_ARG, "query band too tall for one launch");
  return launch_kernel(&dist_kernel<TQ, NW, MODE, PackT>, dim3((unsigned)p.n_rtiles, (unsigned)q_tiles), dim3(NW * 64),
                       name, a, p, s);
}

// The grid of the 256 x 32 tile kernels over the band: fills p's grid fields (q_tile0, r_limit, the strip, r_tiles /
// q_tiles, xcd_*, n_strip_pad, tri_*, n_tiles, tiles_per_xcd) and gives the workgroups along x in *n_blocks_out (0: the
// band holds no tile).  nw: wavefronts per workgroup; strips: the mode has strip tiles; one_order: an instantiation
// without the A/B tile orders.
int plan_grid(DistParams &p, int nw, bool strips, bool one_order, const PpkGeometry &geo, size_t *n_blocks_out) {
  *n_blocks_out = 0;
  const int qt = nw * V2_TQ;
  p.q_tile0 = p.q_begin / qt;
  const size_t q_tiles = (p.q_end + qt - 1) / qt - p.q_tile0;
  size_t r_tiles = (p.n_ref + V2_RT - 1) / V2_RT;
  p.r_limit = p.n_ref;
  p.n_strip = 0;
  p.strip_rt0 = 0;
  p.strip_r_tiles = 1;
  p.strip_begin = p.n_ref;

  // Ragged right edge of the self job: when n_ref is a little over a multiple of 256, the last
  // ref tile would pair its few valid refs with EVERY query tile (n = 10 000: 16 refs, 313 tiles,
  // 4.5 % of all compare work).  Those refs are handled instead by "strip" tiles in which they
  // sit on the query axis against all smaller samples on the lane axis, writing the same
  // condensed rows; the strip tiles lead the same grid.
  const size_t rem = p.n_ref % V2_RT;
  if (strips) {
    bool split = p.self && rem != 0 && rem <= 224 && p.n_ref > V2_RT;
#ifdef PPK_EXPERIMENTS
    if (ppk_config().strip.load() == 0) split = false;
#endif
    if (split) {
      p.r_limit = p.n_ref - rem;
      p.strip_begin = p.r_limit;
      r_tiles = p.r_limit / V2_RT;
      p.strip_rt0 = (unsigned)(p.q_begin / V2_RT);          // lane tiles intersecting the band's rows
      const size_t rt_hi = ((p.q_end < p.n_ref ? p.q_end : p.n_ref) + V2_RT - 1) / V2_RT;
      p.strip_r_tiles = (unsigned)(rt_hi - p.strip_rt0);
      p.n_strip = p.strip_r_tiles * (unsigned)((rem + qt - 1) / qt);
    }
  }
  if (q_tiles == 0 || (r_tiles == 0 && p.n_strip == 0)) return PPK_OK;
  p.r_tiles = (unsigned)(r_tiles ? r_tiles : 1);
  p.q_tiles = (unsigned)(r_tiles ? q_tiles : 0);
  p.xcd_map = 0;      // XCD-contiguous runs
#ifdef PPK_EXPERIMENTS
  p.xcd_map = (int)ppk_config().map.load();  // A/B of tile orders
#endif
  if (p.k_split || one_order) p.xcd_map = 0;      // (the alternatives exist in the EXP instantiation only)
  const unsigned xcds = 1u << geo.xcd_shift;
  p.xcd_shift = geo.xcd_shift;
  p.n_strip_pad = (p.n_strip + xcds - 1u) & ~(xcds - 1u);
  p.tri_m = V2_RT / qt;
  p.tri_c0 = p.tri_m - (int)p.q_tile0;
  const unsigned long long n_tiles64 = r_tiles ? tiles_before64(p.r_tiles, p.self, p.q_tiles, p.tri_m, p.tri_c0) : 0;
  if (n_tiles64 > 0x7ffffff0ull) return ppk_fail(PPK_ERR_ARG, "tile grid too large for one launch: split the query band");
  p.n_tiles = (unsigned)n_tiles64;
  p.tiles_per_xcd = (p.n_tiles + xcds - 1u) / xcds;
  // A/B orders: 1 = XCD-owned interleaved streams (each as long as the busiest XCD's list),
  // 2 = plain (ref tile fastest, skewed for the self job)
  const size_t per_xcd = ((r_tiles + 7) / 8) * q_tiles;
  const size_t n_tri = !r_tiles ? 0 : p.xcd_map == 0 ? (size_t)p.tiles_per_xcd * xcds
                                  : p.xcd_map == 1 ? per_xcd * 8 : r_tiles * q_tiles;
  const size_t n_blocks = n_tri + p.n_strip_pad;
  if (n_blocks * (size_t)(nw * 64) >= ((size_t)1 << 32))
    return ppk_fail(PPK_ERR_ARG, "internal: tile grid too large for one launch (ppk_launch_dist splits bands before this)");
  *n_blocks_out = n_blocks;
  return PPK_OK;
}

// k-split job in one launch: ks_units workgroups per tile, the last one to finish fits it (KS_FUSED in the
// kernel).  Scratch: one zero-initialised counter per tile; 32 bytes per (tile, unit, thread) of partial counts.
template <int NW, int MODE, bool WIDE>
int launch_ksplit_fused(int dev, const DistArgs &a, DistParams &p, size_t n_blocks, hipStream_t s) {
  void *d_tickets = nullptr, *d_part = nullptr;
  const size_t ticket_bytes = (n_blocks * 4 + 255) / 256 * 256;
  int rc = ppk_scratch_get(dev, SLOT_TICKETS, ticket_bytes, &d_tickets);
  if (rc != PPK_OK) return kNoKsplitScratch;
  rc = ppk_scratch_get(dev, SLOT_ITER_A, n_blocks * (size_t)p.ks_units * (NW * 64) * 32 + 256, &d_part);
  if (rc != PPK_OK) return kNoKsplitScratch;
  p.ks_part_off = (size_t)(static_cast<char *>(d_part) - static_cast<char *>(d_tickets));
  p.ks_tickets = static_cast<unsigned *>(d_tickets);
  const char *name = WIDE ? "dist_kernel_v2<256x32,lds-dma,k-split fused,fit from parts>" : "dist_kernel_v2<256x32,lds-dma,k-split fused>";
#ifdef PPK_EXPERIMENTS
  if constexpr (!WIDE && MODE == MODE_DIST)
    if (p.ablate)
      return launch_kernel(&dist_kernel_v2<NW, MODE, 2, true, false, true>, dim3((unsigned)n_blocks, p.ks_units),
                           dim3(NW * 64), name, a, p, s);
#endif
  // Option "ks_grid_pad": one more (empty) column of workgroups.  gridDim.x is otherwise a multiple of 8 and
  // workgroups go to XCD (linear id mod 8), so the ks_units workgroups of a tile all run on ONE XCD and the
  // hand-over below never crosses an L2; with an odd width unit y of tile x runs on XCD (x + y) mod 8
  // (tools/ubench_grid_xcd.hip).  The extra workgroups return at once (their j is past tiles_per_xcd).
  const unsigned grid_x = (unsigned)n_blocks + (ppk_config().ks_grid_pad.load() != 0 ? 1u : 0u);
  return launch_kernel(&dist_kernel_v2<NW, MODE, 2, true, WIDE>, dim3(grid_x, p.ks_units), dim3(NW * 64), name, a, p, s);
}

// More than 128 count bits per pair: the four-dword register windowed over the k list, full windows parked in
// the spill-slot pool (PackWide): a bitmap page + nslots x groups x 128 KB, kept per device
template <int NW, int MODE>
int launch_wide(int dev, const PpkGeometry &geo, const DistArgs &a, DistParams &p, size_t n_blocks, hipStream_t s) {
  p.wide_kpg = 128 / p.cnt_bits;
  if (const long long force = ppk_config().wide_kpg.load(); force > 0 && force < p.wide_kpg) p.wide_kpg = (int)force;
  p.wide_groups = (p.nk + p.wide_kpg - 1) / p.wide_kpg;
  // spill slots: a power of two, at least twice the workgroups the device holds at once
  p.wide_nslots = 64;
  while (p.wide_nslots < 2u * (unsigned)geo.tile_slots) p.wide_nslots *= 2;
  void *pool = nullptr;
  const size_t pool_bytes = 4096 + (size_t)p.wide_nslots * (size_t)p.wide_groups * WIDE_GROUP_U64 * 8;
  int rc = ppk_scratch_get(dev, SLOT_WIDE, pool_bytes, &pool);
  if (rc != PPK_OK) return rc;
  p.wide_bitmap = static_cast<unsigned *>(pool);
  p.wide_slots = reinterpret_cast<unsigned long long *>(static_cast<char *>(pool) + 4096);
  // every launch leaves the bitmap at zero -- unless one was aborted in a process that lives on: a bit left set
  // would make a later workgroup wait for a slot nobody returns.  The pool is idle here (a scratch slot last used
  // on another stream has been waited for), so the page is simply cleared again.
  PPK_HIP(hipMemsetAsync(pool, 0, 4096, s));
  return launch_kernel(&dist_kernel_v2<NW, MODE, 4, false, true>, dim3((unsigned)n_blocks), dim3(NW * 64),
                       "dist_kernel_v2<256x32,lds-dma,wide>", a, p, s);
}

// A self job on a rank-coded database (ppk_db_create) compares the codes: 8, 10 or 12 planes per block instead of
// 14, the same counts.  (ref x query jobs would need one code for two databases; k-split jobs have their own kernels.)
// The pairs (PpkCodingKind) serve the triangular job alone: every pair it compares is two different samples, one from
// each copy; the latest kind the database holds and the options allow is read.  A rectangular job of a handle against
// itself has the pairs (r, r), where a value with a single holder must match itself: it reads the injective copy if
// there is one, else the raw planes.  Returns the coding this band reads (null: the raw planes).
const PpkCoding *coded_planes(const ppk_db *ref, const ppk_db *qry, const DistParams &p) {
  if (!(p.self || qry == ref) || p.k_split || !ppk_coding_enabled(PPK_CODING_RANK)) return nullptr;
  for (int kind = PPK_CODING_FOLDH; p.self && kind > PPK_CODING_RANK; --kind)
    if (ref->coding[kind].planes != 0 && ppk_coding_enabled(kind)) return &ref->coding[kind];
  const PpkCoding &injective = ref->coding[PPK_CODING_RANK];
  return injective.d_ref ? &injective : nullptr;
}
template <int MODE>
int launch_rank(const PpkCoding &c, DistArgs a, DistParams &p, size_t n_blocks, hipStream_t s) {
  a.sk_r = c.d_ref;
  a.sk_q = c.d_qry;
  ppk_coding_launch_flags(c, p.rank_short, p.fold2_six);
  // (the holder pair's 32-bit entries travel in the event list's fields: dist_kernel_v2_foldh reads them as such)
  p.fold2_ev = static_cast<const uint16_t *>(c.d_list);
  p.fold2_off = c.d_off;
  p.fold2_rt = c.rt;
  static const char *const suffix[PPK_CODINGS] = {">", ",fold>", ",fold2>", ",foldh>"};
  auto pick = [&c]() {
    if constexpr (ppk_is_rows(MODE))      // (kernels of their own names: the others keep their instantiations)
      return c.kind == PPK_CODING_FOLDH   ? &dist_kernel_v2_fold_rows<MODE, true>
             : c.kind == PPK_CODING_FOLD2 ? &dist_kernel_v2_fold_rows<MODE, false>
             : c.planes == 12             ? &dist_kernel_v2_rank_rows<12, MODE>
             : c.planes == 10             ? &dist_kernel_v2_rank_rows<10, MODE>
                                          : &dist_kernel_v2_rank_rows<8, MODE>;
    else
      return c.kind == PPK_CODING_FOLDH   ? &dist_kernel_v2_foldh<MODE>
             : c.kind == PPK_CODING_FOLD2 ? &dist_kernel_v2_fold2<MODE>
             : c.planes == 12             ? &dist_kernel_v2_rank<12, MODE>
             : c.planes == 10             ? &dist_kernel_v2_rank<10, MODE>
                                          : &dist_kernel_v2_rank<8, MODE>;
  };
  const auto kernel = pick();
  std::string name = "dist_kernel_v2<256x32,lds-dma,rank " + std::to_string(c.planes) + suffix[c.kind];
  if (ppk_is_rows(MODE)) name.insert(name.size() - 1, ",rows");
  return launch_kernel(kernel, dim3((unsigned)n_blocks), dim3(8 * 64), name.c_str(), a, p, s);
}

// One band through the 256 x 32 tile kernels: the grid, then the variant that p and the instantiation select
template <int NW, int MODE, int W, bool WIDE = false>
int launch_v2(const ppk_db *ref, const ppk_db *qry, const DistArgs &a, DistParams &p, hipStream_t s) {
  constexpr bool kFits = MODE == MODE_DIST || ppk_is_mask(MODE);      // the modes that fit a pair in the tile's epilogue
  const PpkGeometry &geo = ppk_geometry(ref->device);
  size_t n_blocks = 0;
  // (the rows modes reserve staging per mask word, and a strip tile sets single bits of other tiles' words: no strips)
  const int rc = plan_grid(p, NW, kFits && !ppk_is_rows(MODE), WIDE, geo, &n_blocks);
  if (rc != PPK_OK || n_blocks == 0) return rc;
  if constexpr (ppk_is_rows(MODE)) {
    // whole tiles of the plain packed kernels only: ppk_edge_rows_fused has sent every other shape through the two-step
    if (p.k_split || WIDE) return ppk_fail(PPK_ERR_STATE, "internal: the rows modes have whole-tile instantiations only");
  }
  if (kFits && NW == 8 && p.k_split) {
    if constexpr (NW == 8 && W == 2 && kFits && !ppk_is_rows(MODE))
      return launch_ksplit_fused<NW, MODE, WIDE>(ref->device, a, p, n_blocks, s);
    return ppk_fail(PPK_ERR_STATE, "internal: no k-split instantiation for this mode");
  }
  if constexpr (WIDE && W != 4) {
    return ppk_fail(PPK_ERR_STATE, "internal: the fit-from-parts instantiation is a k-split kernel");
  } else if constexpr (WIDE && !ppk_is_rows(MODE)) {
    return launch_wide<NW, MODE>(ref->device, geo, a, p, n_blocks, s);
  }
  const dim3 grid((unsigned)n_blocks), block(NW * 64);
#ifdef PPK_EXPERIMENTS
  // the experiments build (make experiments): `ablate` and the rejected tile orders run their own instantiation
  if ((p.ablate || p.xcd_map) && !p.k_split)
    return launch_kernel(&dist_kernel_v2<NW, MODE, W, false, false, true>, grid, block, "dist_kernel_v2<256x32,lds-dma,exp>", a, p, s);
#endif
  if constexpr (NW == 8 && W == 2 && !WIDE && kFits) {
    if (const PpkCoding *c = coded_planes(ref, qry, p)) return launch_rank<MODE>(*c, a, p, n_blocks, s);
  }
  // (the counts pass of a two-pass k-split job: one workgroup per (tile, k))
  if constexpr (MODE == MODE_COUNTS && NW == 8)
    if (p.k_split)
      return launch_kernel(&dist_kernel_v2<NW, MODE, W, true>, dim3((unsigned)n_blocks, (unsigned)p.nk), block,
                           "dist_kernel_v2<256x32,lds-dma>", a, p, s);
  return launch_kernel(&dist_kernel_v2<NW, MODE, W>, grid, block,
                       ppk_is_rows(MODE) ? "dist_kernel_v2<256x32,lds-dma,rows>" : "dist_kernel_v2<256x32,lds-dma>", a, p, s);
}

// COUNTS / JACCARD modes: each k's counts are consumed at once, nothing is packed
template <int MODE>
int launch_tiles_unpacked(const ppk_db *ref, const ppk_db *qry, const DistArgs &a, DistParams &p, hipStream_t s) {
  static_assert(MODE == MODE_COUNTS || MODE == MODE_JACCARD, "unpacked modes");
  if (p.bbits != 14) return launch_variant<8, 4, MODE, uint64_t>(a, p, s, "dist_kernel<8,4,generic>");
  return launch_v2<8, MODE, 1>(ref, qry, a, p, s);
}

// DIST / MASK modes: the per-pair count register is sized by nk * cnt_bits (<= 128, checked by
// the caller)
template <int MODE>
int launch_tiles_packed(const ppk_db *ref, const ppk_db *qry, const DistArgs &a, DistParams &p, hipStream_t s) {
  static_assert(MODE == MODE_DIST || ppk_is_mask(MODE) || MODE == MODE_KNN, "packed modes");
  const int total_bits = p.nk * p.cnt_bits;
  if constexpr (MODE == MODE_KNN) {
    if (p.bbits != 14) return ppk_fail(PPK_ERR_ARG, "neighbours from tiles need bbits = 14 (use the square-matrix path)");
  } else if (p.bbits != 14) {
    // the generic-bbits kernel has registers to spare and packs into plain integers
    if (total_bits <= 64) return launch_variant<8, 4, MODE, uint64_t>(a, p, s, "dist_kernel<8,4,generic>");
    if (p.nk <= 6 && p.cnt_bits <= 16) return launch_variant<8, 4, MODE, Pack96>(a, p, s, "dist_kernel<8,4,generic>");
    return launch_variant<8, 4, MODE, u128>(a, p, s, "dist_kernel<8,4,generic>");
  }
  // (option "wide_kpg": a narrower window, i.e. the wide path on a k list the register would hold -- tests)
  const long long force_kpg = ppk_config().wide_kpg.load();
  if constexpr (MODE == MODE_DIST || ppk_is_mask(MODE)) {
    // a k-split job whose tiles are fitted from the units' partial counts as they lie (any k list)
    // (every k list of more than 64 count bits: rebuilding three- and four-dword registers in the last unit measured
    // the same -- profiles/r05/ksplit_fit_from_parts.txt -- and cost two more instantiations, both with spills; the
    // two-dword register path stays for the shapes whose tiles are fitted from the LDS table)
    if (p.k_split && (total_bits > 64 || (force_kpg > 0 && force_kpg < p.nk))) return launch_v2<8, MODE, 2, true>(ref, qry, a, p, s);
    if (p.k_split) return launch_v2<8, MODE, 2>(ref, qry, a, p, s);
  }
  if (total_bits > 128 || (force_kpg > 0 && force_kpg < p.nk && !p.k_split)) return launch_v2<8, MODE, 4, true>(ref, qry, a, p, s);
  if (total_bits <= 64) return launch_v2<8, MODE, 2>(ref, qry, a, p, s);
  if (total_bits <= 96) return launch_v2<8, MODE, 3>(ref, qry, a, p, s);
  return launch_v2<8, MODE, 4>(ref, qry, a, p, s);
}

// MASK_ROWS / BGMM_ROWS modes: whole tiles of the three packed count registers, nothing else (the caller has asked
// ppk_edge_rows_fused, and a band that would go k-split on its own runs whole tiles here -- the same bits)
template <int MODE>
int launch_tiles_rows(const ppk_db *ref, const ppk_db *qry, const DistArgs &a, DistParams &p, hipStream_t s) {
  static_assert(ppk_is_rows(MODE), "rows modes");
  const int total_bits = p.nk * p.cnt_bits;
  const long long force_kpg = ppk_config().wide_kpg.load();
  if (p.bbits != 14 || p.k_split || total_bits > 128 || (force_kpg > 0 && force_kpg < p.nk))
    return ppk_fail(PPK_ERR_STATE, "internal: this shape takes the two-step (ppk_edge_rows_fused)");
  if (total_bits <= 64) return launch_v2<8, MODE, 2>(ref, qry, a, p, s);
  if (total_bits <= 96) return launch_v2<8, MODE, 3>(ref, qry, a, p, s);
  return launch_v2<8, MODE, 4>(ref, qry, a, p, s);
}

}  // namespace

// Whether the edge calls with rows (ppk_dist_edges_rows_dev / ppk_dist_bgmm_edges_rows_dev) emit the rows from the tile
// kernel's own epilogue for this band, or run the two-step (the edge call, then the list kernel on its edges: the same
// bits).  The one place that decides: fused on the plain packed whole-tile route -- bbits 14, at most 128 count bits, no
// forced wide window, and a band the route choice sends through whole tiles.  Option "edge_rows_fused" 0 forces the
// two-step.
bool ppk_edge_rows_fused(const ppk_db *ref, const ppk_db *qry, size_t q_begin, size_t q_end) {
  if (ppk_config().edge_rows_fused.load() == 0 || ppk_unfused(ref) || ref->bbits != V2_BB || ref->nk < 1) return false;
  const int bits = count_bits(ref->s64);
  const long long force_kpg = ppk_config().wide_kpg.load();
  if (ref->nk * (size_t)bits > 128 || (force_kpg > 0 && force_kpg < (long long)ref->nk)) return false;
  const int self = qry ? 0 : 1;
  const size_t rows = ppk_rows_in_band(ref->n, qry ? qry->n : 0, q_begin, q_end);
  PpkRouteShape shape = {ref->n, q_end - q_begin, rows, self, (int)ref->nk, (int)ref->s64, bits, (int)ref->bbits, 1, 0};
  return ppk_choose_route_impl(shape, ppk_geometry(ref->device), route_knobs()).route == PPK_ROUTE_TILE;
}

int ppk_launch_transpose(const uint64_t *d_in, uint64_t *d_out, size_t n, size_t cols, size_t npad,
                         hipStream_t s) {
  dim3 grid((unsigned)((cols + 31) / 32), (unsigned)(npad / 32));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, s, d_in, d_out, n, cols, npad);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

// whether a self job over the whole of `db` runs whole 256 x 32 tiles of the two-dword count register under the
// options in force: the one shape that reads a rank-coded copy (launch_v2)
bool ppk_self_job_takes_tiles(const ppk_db *db) {
  if (db->bbits != V2_BB || db->n < 2) return false;
  const int bits = count_bits(db->s64);
  if (db->nk * (size_t)bits > 64) return false;
  PpkRouteShape shape = {db->n, db->n, db->n * (db->n - 1) / 2, 1, (int)db->nk, (int)db->s64, bits, (int)db->bbits, 0, 0};
  return ppk_choose_route_impl(shape, ppk_geometry(db->device), route_knobs()).route == PPK_ROUTE_TILE;
}

// ---- device geometry -----------------------------------------------------------------------------------------------
// Nothing below assumes a part: the compute units, the XCD count and the number of pair-tile workgroups the device
// holds at once are read here, once per device (ppk_geometry keeps the answer).  (MI355X in SPX mode: 256 CUs, 8 XCDs,
// 2 workgroups of the tile kernel per CU = 512 slots; in CPX mode one partition shows 32 CUs, 1 XCD, 64 slots.)
PpkGeometry ppk_measure_geometry(int dev) {
  PpkGeometry g = {256, 3, 512};      // (what a whole MI355X shows, for whatever cannot be read)
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) g.cus = v;
  unsigned shift = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeNumberOfXccs, dev) == hipSuccess && v > 0) {
    while ((2u << shift) <= (unsigned)v) ++shift;
  } else {
    shift = g.cus >= 64 ? 3 : 0;      // (attribute missing: eight XCDs is what a whole MI300 / MI355X shows)
  }
  g.xcd_shift = shift;
  int per_cu = 0;
  DeviceGuard guard(dev);
  if (guard.ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(
                      &per_cu, reinterpret_cast<const void *>(&dist_kernel_v2<8, MODE_DIST, 2, false, false>), 512, 0) == hipSuccess &&
      per_cu > 0)
    g.tile_slots = per_cu * g.cus;
  else
    g.tile_slots = 2 * g.cus;
  return g;
}

// ---- the route of one band --------------------------------------------------------------------------------------------
// A pure function of the job's shape, the device's geometry and the options: which of the kernel shapes of DESIGN.md
// section 3.1 a band of pair tiles runs through.  Tile-count rules were measured on 512 workgroup slots (MI355X, SPX) and
// are stated in those units; `rounds()` rescales them to the slots this device has.  tests/test_host_logic.py pins the
// choices on MI355X for the shapes of profiles/r05/ksplit_*.txt and checks a CPX-shaped geometry picks sanely.
PpkRouteChoice ppk_choose_route_impl(const PpkRouteShape &sh, const PpkGeometry &g, const PpkRouteKnobs &kn) {
  PpkRouteChoice c = {};
  c.route = PPK_ROUTE_TILE;
  c.slices = 1;
  auto rounds = [&](size_t tiles_at_512) { return tiles_at_512 * (size_t)g.tile_slots / 512; };
  const size_t rt = (sh.n_ref + V2_RT - 1) / V2_RT, qt = (sh.q_rows + 31) / 32;
  const size_t tiles = sh.self ? rt * qt / 2 + qt : rt * qt;
  c.tiles = tiles;
  // more than 128 count bits per pair: the tile kernel's WIDE instantiation (bbits = 14); other bbits (never
  // written by PopPUNK: sketchlib fixes bbits = 14) keep the two-pass counts route for plain distances
  const bool too_wide = sh.nk > PPK_MAX_NK || (sh.nk * sh.cnt_bits > 128 && sh.bbits != 14);
  if (too_wide) {
    c.route = PPK_ROUTE_COUNTS_UNFUSED;
    return c;
  }
  const bool wide_tile = sh.nk * sh.cnt_bits > 128 || (kn.wide_kpg > 0 && kn.wide_kpg < sh.nk);
  if (wide_tile && sh.bbits == 14) c.route = PPK_ROUTE_TILE_WIDE;
  // Small jobs (up to about one round of pair tiles on the device's workgroup slots, e.g. 1 000 genomes or a handful
  // of queries): one workgroup per (tile, k) instead of per tile -- nk times the parallelism, a serial chain of s64
  // blocks instead of nk * s64.  (The fused boundary mode takes the path in its one-launch form only.)
  const bool one_launch_ok = kn.ksplit_fused != 0 && 64 * (size_t)sh.s64 < 65536;
  const bool edge_ks = sh.mask && one_launch_ok && sh.s64 >= 2;
  if ((sh.mask && !edge_ks) || sh.knn || sh.bbits != 14 || sh.nk < 2) return c;
  // default 1 200 tiles at 5 k since the one-launch form (round 4; profiles/r04/ksplit_threshold*.txt: it wins by
  // 10 - 50 % up to 4 000 genomes / 1 125 tiles and ties from there to 1 800 tiles; 215 with the two-pass form),
  // scaled by 5 / nk: the comparison is between nk * tiles short workgroups and `tiles` long ones.  The raised
  // threshold holds where it was measured: sketches whose tiles are fitted from the LDS table -- 3 to 5 k of 11-bit
  // counts, i.e. s = 1024.  Other shapes fit a tile with the general statement, a long tail for a k-split tile.
  const bool lds_fit = sh.nk >= 3 && sh.nk <= 5 && sh.cnt_bits == 11;
  long long ks = kn.ksplit;      // tile-count threshold at 5 k (for 512 slots), 0 = off
  if (!lds_fit && ks > kn.ksplit_wide) ks = kn.ksplit_wide;
  size_t limit = ks > 0 ? rounds((size_t)ks) * 5 / (size_t)sh.nk : 0;
  // s = 1 024 with a k list the LDS table does not serve (6 k and up): in TILES the crossover does not move with nk
  // (profiles/r05/ksplit_s1024_other_shapes.txt): level at 1 125 tiles, behind from 6 000 genomes
  if (!lds_fit && ks > 0 && sh.s64 >= 16 && limit < rounds(700) && kn.ksplit_wide >= 215) limit = rounds(700);
  // LONG sketches (sketchsize64 >= 32; PopPUNK's default is 156): a pair tile is a serial chain of nk * s64 blocks,
  // so whole tiles fill the last round of workgroup slots badly at ANY job size, and they cycle through every k's
  // rows while a k-split job works through the database one k at a time (profiles/r05/ksplit_long_sketches.txt).
  // The path is taken whenever its scratch stays within `scratch_cap`: the partial counts, 16 KB per (tile, unit)
  // with the grid's padding counted (a column per XCD and the ragged edge's strip), or 4 B per (row, k) in the
  // two-pass form.  Option "ksplit_long" 0 restores the tile-count rule above.
  int slices = 1;
  {
    // Very small jobs still leave workgroup slots empty with one workgroup per (tile, k): each k is cut into 2 or 4
    // pieces of consecutive blocks as long as that stays within one round of the slots.
    const size_t wgs = tiles * (size_t)sh.nk;
    while (slices < 4 && wgs * (size_t)slices * 2 <= (size_t)g.tile_slots && sh.s64 % (slices * 2) == 0) slices *= 2;
    if (kn.ksplit_slices > 0 && kn.ksplit_slices <= 4 && sh.s64 % kn.ksplit_slices == 0) slices = (int)kn.ksplit_slices;
    // a unit of ONE block would re-fetch the block behind its range: one launch needs units of two blocks
    if (kn.ksplit_fused != 0)
      while (slices > 1 && sh.s64 / slices < 2) slices /= 2;
  }
  const size_t xcds = (size_t)1 << g.xcd_shift;
  const size_t strip_tiles = sh.self ? (rt + 1) * ((V2_RT + 31) / 32) : 0;      // (upper bound: the strip of a ragged edge)
  // (a band of the triangle can hold up to rt * qt tiles: the estimate above is for the whole triangle)
  const size_t grid_cols = (sh.self && sh.q_rows >= sh.n_ref ? tiles : rt * qt) + 2 * xcds + strip_tiles + 1;
  const size_t one_launch_scratch = grid_cols * (size_t)sh.nk * (size_t)slices * (16 << 10);
  if (ks > 0 && sh.s64 >= 32 && kn.ksplit_long != 0) {
    const size_t scratch = one_launch_ok ? one_launch_scratch : sh.rows * (size_t)sh.nk * 4;
    // (the two-pass form's fit pass costs 0.2 us per 1 000 rows at 10 k: it pays up to about 700 tiles)
    if (scratch <= kn.scratch_cap && (sh.s64 >= 64 || tiles <= rounds(6600)) && (one_launch_ok || tiles <= rounds(700)))
      limit = tiles;
  }
  c.limit = limit;
  if (tiles > limit) return c;
  // ---- a k-split job ----
  c.slices = slices;
  const int ks_blocks = sh.s64 / slices;
  c.from_parts = sh.nk * sh.cnt_bits > 64 || (kn.wide_kpg > 0 && kn.wide_kpg < sh.nk);
  if (kn.ksplit_fused != 0 && ks_blocks >= 2 && 64 * (size_t)ks_blocks < 65536 &&
      (!c.from_parts || 64 * (size_t)sh.s64 < 65536)) {
    if (one_launch_scratch > kn.scratch_cap) return c;      // (does not fit what may be taken: the tile kernel needs none)
    c.route = PPK_ROUTE_KSPLIT_ONE_LAUNCH;
    c.scratch_bytes = one_launch_scratch;
    return c;
  }
  if (sh.mask) return c;      // (cannot happen: edge_ks admits one-launch shapes only; stay on the tile kernel)
  c.route = PPK_ROUTE_KSPLIT_TWO_PASS;
  c.scratch_bytes = sh.rows * (size_t)sh.nk * (size_t)slices * 4;
  return c;
}

// The same through the C ABI (tests on a machine without a GPU: nothing here touches a device)
extern "C" int ppk_choose_route(size_t n_ref, size_t q_rows, int self, int nk, int sketchsize64, int bbits, int mask,
                                int knn, int cus, int xcds, int tile_slots, const long long *knobs, int *route,
                                int *slices, size_t *tiles, size_t *limit) {
  if (!knobs || !route) return ppk_fail(PPK_ERR_ARG, "ppk_choose_route: NULL argument");
  if (nk < 1 || sketchsize64 < 1 || cus < 1 || xcds < 1 || tile_slots < 1) return ppk_fail(PPK_ERR_ARG, "ppk_choose_route: bad shape");
  PpkRouteShape sh = {};
  sh.n_ref = n_ref;
  sh.q_rows = q_rows;
  sh.self = self;
  sh.rows = self ? (q_rows * n_ref - q_rows * (q_rows + 1) / 2) : q_rows * n_ref;
  sh.nk = nk;
  sh.s64 = sketchsize64;
  sh.bbits = bbits;
  sh.cnt_bits = count_bits((size_t)sketchsize64);
  sh.mask = mask;
  sh.knn = knn;
  PpkGeometry g = {cus, 0, tile_slots};
  while ((2u << g.xcd_shift) <= (unsigned)xcds) ++g.xcd_shift;
  PpkRouteKnobs kn = {knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5], (size_t)knobs[6]};
  const PpkRouteChoice c = ppk_choose_route_impl(sh, g, kn);
  *route = c.route;
  if (slices) *slices = c.slices;
  if (tiles) *tiles = c.tiles;
  if (limit) *limit = c.limit;
  return PPK_OK;
}

size_t ppk_rows_per_dispatch(const ppk_db *ref) {
  const size_t r_tiles = (ref->n + V2_RT - 1) / V2_RT;
  long long per_launch = ppk_config().launch_tiles.load();
  if (per_launch < 1 || per_launch > 8000000) per_launch = 8000000;
  size_t q_sub = ((size_t)per_launch / (r_tiles ? r_tiles : 1)) * 32 / 64 * 64;      // 32 query rows per tile
  if (ref->bbits != 14 && q_sub > ((size_t)1 << 17)) q_sub = (size_t)1 << 17;   // generic kernel: 2-D grid, y < 65 536
  return q_sub < 64 ? 64 : q_sub;
}

// What the fit of every route reads of a (database, k list, random table) job: the shape, the table strides, the
// k-mer lengths, the [EXT] switches, and the weights of the all-k-usable fast path (FitCoef)
static void fit_params(const ppk_db *ref, const int32_t *kmers, size_t n_clu, int flags, const float *d_rtab,
                       DistParams &p, FitCoef &coef) {
  p.nk = (int)ref->nk;
  p.s64 = (int)ref->s64;
  p.bbits = (int)ref->bbits;
  const size_t nbins = ref->s64 * 64;
  p.lut_kstride = nbins + 1;
  p.lut_cpstride = (size_t)p.nk * (nbins + 1);
  p.n_clu = (int)(n_clu ? n_clu : 1);
  p.random_correct = (flags & PPK_FLAG_RANDOM_CORRECT) && d_rtab ? 1 : 0;
  p.cnt_bits = count_bits(ref->s64);
  for (int k = 0; k < p.nk && k < PPK_MAX_NK; ++k) p.kmers[k] = kmers[k];
  {
    double sx = 0.0, sxx = 0.0;
    for (int k = 0; k < p.nk && k < PPK_MAX_NK; ++k) {
      sx += (double)kmers[k];
      sxx += (double)kmers[k] * (double)kmers[k];
    }
    const double dn = (double)p.nk, den = dn * sxx - sx * sx;
    for (int k = 0; k < p.nk && k < PPK_MAX_NK; ++k) {
      coef.a[k] = den != 0.0 ? (dn * (double)kmers[k] - sx) / den : 0.0;
      coef.b[k] = (1.0 - coef.a[k] * sx) / dn;
    }
  }
  p.lut_total = (size_t)p.n_clu * p.n_clu * p.lut_cpstride;
  p.lut32 = (p.lut_total * 16 < ((size_t)1 << 32)) ? 1 : 0;
  p.ext_adjust = ppk_config().ext_collision_adjust.load() ? 1 : 0;
  p.ext_skip = ppk_config().ext_fit_skip.load() ? 1 : 0;
}
// the log-J and (E, F) tables of such a job into d_lut (stage_tables found no identical earlier call's there)
static int enqueue_lut(const ppk_db *ref, double *d_lut, const float *d_rtab, const DistParams &p, const FitCoef &coef,
                       hipStream_t s) {
  const size_t total = (size_t)p.n_clu * p.n_clu * p.lut_cpstride;
  hipLaunchKernelGGL(lut_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_lut, d_rtab, p.nk, p.n_clu,
                     ref->s64 * 64, ref->s64, ref->bbits, p.random_correct, p.ext_adjust, total, coef);
  PPK_HIP(hipGetLastError());
  ppk_lut_commit(ref->device, d_lut);
  return PPK_OK;
}

// Kernel 1 for one band that a single dispatch holds
static int launch_dist_band(const DistJob &job) {
  const ppk_db *ref = job.ref, *qry = job.qry ? job.qry : ref;
  const int32_t *kmers = job.kmers;
  hipStream_t s = job.s;
  DistParams p = {};
  p.self = job.qry ? 0 : 1;
  p.npad_r = ref->npad;
  p.npad_q = qry->npad;
  p.n_ref = ref->n;
  p.q_begin = job.q_begin;
  p.q_end = job.q_end;
  p.row_base = p.self ? p.q_begin * ref->n - (p.q_begin * (p.q_begin + 1)) / 2 : p.q_begin * ref->n;
  FitCoef coef = {};
  fit_params(ref, kmers, job.n_clu, job.flags, job.d_rtab, p, coef);
  p.n_rtiles = (ref->n + 63) / 64;
  p.slope = job.slope;
  p.inclusive = job.inclusive;
  p.x_max = job.x_max;
  p.y_max = job.y_max;
  p.scale_x = job.scale_x;
  p.scale_y = job.scale_y;
  p.knn = job.knn_args ? job.knn_args[0] : 0;
  p.knn_col = job.knn_args ? job.knn_args[1] : 0;
  p.ablate = 0;
#ifdef PPK_EXPERIMENTS
  p.ablate = (int)ppk_config().ablate.load();
#endif
  p.lds_table = ppk_config().lds_table.load() != 0 && !(p.ablate & 32) ? 1 : 0;
  p.rows_stage = static_cast<float2 *>(job.d_rows_stage);
  p.rows_base = job.d_rows_base;
  p.rows_count = job.d_rows_count;
  p.rows_cap = job.rows_cap;
  if (job.d_rows_stage && !(job.d_mask && job.d_rows_base && job.d_rows_count))
    return ppk_fail(PPK_ERR_STATE, "internal: a rows launch needs the mask, the word positions and the counter");

  if (job.d_bgmm && !job.d_mask) return ppk_fail(PPK_ERR_STATE, "internal: a BGMM launch needs an edge bitmask");
  // cluster ids only matter when a multi-cluster random-match table is in use
  const bool use_clu = p.random_correct && p.n_clu > 1;
  DistArgs a = {ref->d_skT, qry->d_skT, job.d_lut, use_clu ? ref->d_clu : nullptr, use_clu ? qry->d_clu : nullptr,
                job.d_rtab, job.d_out, job.d_n_failed, job.d_mask};
  // a counts pass: its rows go to scratch, it counts no failures and fills no mask
  auto counts_to = [&a](void *d_cnt) {
    DistArgs c = a;
    c.out = d_cnt, c.n_failed = nullptr, c.mask = nullptr;
    return c;
  };
  if (job.flags & PPK_FLAG_COUNTS) return launch_tiles_unpacked<MODE_COUNTS>(ref, qry, a, p, s);
  if (job.flags & PPK_FLAG_JACCARD) return launch_tiles_unpacked<MODE_JACCARD>(ref, qry, a, p, s);

  // which kernel shape this band runs through: a pure function of shape, geometry and options (ppk_choose_route_impl)
  const size_t rows = band_rows(p);
  PpkRouteShape shape = {ref->n, p.q_end - p.q_begin, rows, p.self, p.nk, p.s64, p.cnt_bits, p.bbits, job.d_mask ? 1 : 0,
                         job.knn_args ? 1 : 0};
  PpkRouteChoice choice = ppk_choose_route_impl(shape, ppk_geometry(ref->device), route_knobs());
  if (choice.route == PPK_ROUTE_COUNTS_UNFUSED) {
    // the packed per-pair state does not fit: raw counts to scratch, then a generic regression pass
    if (job.knn_args) return ppk_fail(PPK_ERR_ARG, "neighbours from tiles need bbits = 14");
    if (job.d_mask) return ppk_fail(PPK_ERR_STATE, "internal: counts fallback is resolved by the caller");
    void *p_cnt = nullptr;
    int rc = ppk_scratch_get(ref->device, SLOT_ITER_A, rows * (size_t)p.nk * 4 + (size_t)p.nk * 4 + 256, &p_cnt);
    if (rc != PPK_OK) return rc;
    uint32_t *d_cnt = static_cast<uint32_t *>(p_cnt);
    int *d_kmers = reinterpret_cast<int *>(d_cnt + rows * (size_t)p.nk);
    PPK_HIP(hipMemcpyAsync(d_kmers, kmers, (size_t)p.nk * 4, hipMemcpyHostToDevice, s));
    rc = launch_tiles_unpacked<MODE_COUNTS>(ref, qry, counts_to(d_cnt), p, s);
    if (rc != PPK_OK) return rc;
    hipLaunchKernelGGL(regress_counts_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, d_cnt,
                       rows, p.row_base, p.self, p.n_ref, p.nk, d_kmers, ref->s64, ref->bbits,
                       p.random_correct ? job.d_rtab : nullptr, p.n_clu, a.rclu, a.qclu, job.scale_x, job.scale_y,
                       p.ext_adjust, p.ext_skip, static_cast<float2 *>(job.d_out), job.d_n_failed);
    PPK_HIP(hipGetLastError());
    return PPK_OK;
  }
  // log-J table, built on the device for this (random table, k list) -- unless an identical earlier call
  // left it there (stage_tables)
  if (!job.lut_ready)
    if (const int rc = enqueue_lut(ref, job.d_lut, job.d_rtab, p, coef, s)) return rc;
  // The band's mode.  MODE_KNN -- d_out: candidate arrays, d_mask: KnnState + bounds over n_ref (+ n_qry: a ref x
  // query job) samples.  MODE_BGMM reads the model through the kernel's `out` pointer (MODE_MASK leaves it unused).
  if (job.d_bgmm) a.out = const_cast<ppk_bgmm *>(job.d_bgmm);
  auto launch_packed = [&]() {
    if (job.knn_args) return launch_tiles_packed<MODE_KNN>(ref, qry, a, p, s);
    if (job.d_rows_stage && job.d_bgmm) return launch_tiles_rows<MODE_BGMM_ROWS>(ref, qry, a, p, s);
    if (job.d_rows_stage) return launch_tiles_rows<MODE_MASK_ROWS>(ref, qry, a, p, s);
    if (job.d_bgmm) return launch_tiles_packed<MODE_BGMM>(ref, qry, a, p, s);
    if (job.d_mask) return launch_tiles_packed<MODE_MASK>(ref, qry, a, p, s);
    return launch_tiles_packed<MODE_DIST>(ref, qry, a, p, s);
  };
  if (choice.route != PPK_ROUTE_KSPLIT_ONE_LAUNCH && choice.route != PPK_ROUTE_KSPLIT_TWO_PASS) return launch_packed();
  // (a short last piece of a rows job that ppk_edge_rows_fused sent through whole tiles: whole tiles too, the same bits)
  if (job.d_rows_stage) return launch_packed();

  // a small job: one workgroup per (tile, k), or per piece of a k (ppk_choose_route_impl)
  const int slices = choice.slices;
  p.k_split = slices;
  p.ks_rows = rows;
  p.ks_blocks = p.s64 / slices;
  p.ks_units = (unsigned)(p.nk * slices);
  if (choice.route == PPK_ROUTE_KSPLIT_ONE_LAUNCH) {
    // ONE launch: every tile's last unit fits it
    // (a unit's counts travel as 16-bit numbers; fitted from the parts as they lie, a k's pieces are added in place)
    const int rc1 = launch_packed();
    if (rc1 != kNoKsplitScratch) return rc1;
    // the device could not give the partial counts their scratch: the band runs through the tile kernel, which
    // needs none (a job that fits a nearly full GPU must not fail on a buffer that only buys speed)
    (void)hipGetLastError();
    p.k_split = 0;
    return launch_packed();
  }
  // two passes: raw counts, k-major, then the same per-pair fit as the tile epilogue
  if (job.d_mask) return ppk_fail(PPK_ERR_STATE, "internal: the two-pass k-split route serves plain distances only");
  void *p_cnt = nullptr;
  int rc = ppk_scratch_get(ref->device, SLOT_ITER_A, rows * (size_t)p.nk * slices * 4 + 256, &p_cnt);
  if (rc != PPK_OK) return rc;
  {
    DistParams pc = p;
    pc.nk = p.nk * slices;
    pc.s64 = p.s64 / slices;
    rc = launch_tiles_unpacked<MODE_COUNTS>(ref, qry, counts_to(p_cnt), pc, s);
  }
  if (rc != PPK_OK) return rc;
  ppk_set_kernel_name("dist_kernel_v2<256x32,lds-dma,k-split counts> + regress_packed_kernel");
  ppk_prof_begin(s);
  hipLaunchKernelGGL(regress_packed_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s,
                     static_cast<const uint32_t *>(p_cnt), rows, job.d_lut, a.rclu, a.qclu,
                     static_cast<float2 *>(job.d_out), job.d_n_failed, p);
  ppk_prof_end(s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

// one band of raw-plane counts of two given copies (the holder pair's temporary pair): the tile kernel in MODE_COUNTS
int ppk_counts_band_raw(const ppk_db *db, const uint64_t *d_r, const uint64_t *d_q, size_t q_begin, size_t q_end, void *d_cnt,
                        hipStream_t s) {
  DistParams p = {};
  p.self = 1;
  p.npad_r = p.npad_q = db->npad;
  p.n_ref = db->n;
  p.q_begin = q_begin;
  p.q_end = q_end;
  p.row_base = q_begin * db->n - (q_begin * (q_begin + 1)) / 2;
  FitCoef coef = {};
  int32_t kmers[PPK_MAX_NK] = {};
  fit_params(db, kmers, 0, 0, nullptr, p, coef);
  p.n_rtiles = (db->n + 63) / 64;
  const DistArgs a = {d_r, d_q, nullptr, nullptr, nullptr, nullptr, d_cnt, nullptr, nullptr};
  return launch_tiles_unpacked<MODE_COUNTS>(db, db, a, p, s);
}
// A dispatch holds fewer than 2^32 work-items: with 512-thread workgroups that is 8.4 M pair tiles, which
// 370 000 genomes against themselves exceed (a million: 61 M).  Larger bands go out as several launches over
// consecutive query rows, each writing to its own part of the output (the kernels address rows and mask
// words relative to the band they are launched on; kNN candidates are appended through a shared counter).
int ppk_launch_dist(const DistJob &job) {
  const ppk_db *ref = job.ref;
  const size_t q_sub = ppk_rows_per_dispatch(ref);
  if (job.q_end - job.q_begin <= q_sub) return launch_dist_band(job);
  const size_t n_qry = job.qry ? job.qry->n : 0;
  const size_t row_bytes = (job.flags & (PPK_FLAG_COUNTS | PPK_FLAG_JACCARD)) ? ref->nk * 4 : 8;
  const size_t n_rtiles = (ref->n + 63) / 64;
  for (size_t lo = job.q_begin; lo < job.q_end; lo += q_sub) {
    const size_t hi = lo + q_sub < job.q_end ? lo + q_sub : job.q_end;
    if (ppk_rows_in_band(ref->n, n_qry, lo, hi) == 0) continue;      // (the last sample of a self job pairs with nobody)
    DistJob band = job;
    band.q_begin = lo;
    band.q_end = hi;
    if (!job.knn_args) {
      if (job.d_out) band.d_out = static_cast<char *>(job.d_out) + ppk_rows_in_band(ref->n, n_qry, job.q_begin, lo) * row_bytes;
      if (job.d_mask) band.d_mask = job.d_mask + (lo - job.q_begin) * n_rtiles;
      if (job.d_rows_base) band.d_rows_base = job.d_rows_base + (lo - job.q_begin) * n_rtiles;
    }
    band.lut_ready = job.lut_ready || lo > job.q_begin;
    const int rc = launch_dist_band(band);
    if (rc != PPK_OK) return rc;
  }
  return PPK_OK;
}

// ---- kernel 1 for a list of pairs -----------------------------------------------------------------------------------
// Check (the call's one synchronisation), then chunk by chunk: mark, gather, count, fit.  Scratch (SLOT_PAIRS): a slot
// word per sample, and per chunk the row image (at most 2 x chunk rows, never more than there are samples) and nk
// counts per pair -- the chunk is sized so that image and counts, as allocated, stay below option "pairs_scratch_mb",
// whatever the list's length.  Stages (ppk_prof_stages names): pairs_check, pairs_image, pairs_counts, pairs_fit.
int ppk_launch_pairs(const PairsJob &job) {
  const ppk_db *ref = job.ref, *qry = job.qry;
  hipStream_t s = job.s;
  const int dev = ref->device;
  const size_t n_ref = ref->n, n_qry = qry ? qry->n : 0, n_tot = n_ref + n_qry, m = job.n_pairs;
  const size_t nk = ref->nk, cols = nk * ref->words, row_bytes = cols * 8;
  if ((n_ref + 31) / 32 > 65535 || (n_qry + 31) / 32 > 65535)
    return ppk_fail(PPK_ERR_ARG, "ppk_dist_pairs: more than 2 097 120 samples in a database");
  const PairsGeom g = {(long long)n_ref, (long long)n_qry, job.int_offset, job.d_i, job.d_j, job.stride};

  // (four fifths of the cap: a scratch slot is allocated with a quarter to spare, and the cap is on what is allocated)
  const long long cap_mb = ppk_config().pairs_scratch_mb.load();
  size_t chunk = ((size_t)(cap_mb > 0 ? cap_mb : 0) << 20) / 5 * 4 / (2 * row_bytes + nk * 4);
  if (const long long force = ppk_config().pairs_chunk.load(); force > 0) chunk = (size_t)force;
  if (chunk < 1) chunk = 1;
  if (chunk > m) chunk = m;
  if (chunk > ((size_t)1 << 30)) chunk = (size_t)1 << 30;      // (slots are 32-bit)
  const size_t img_rows = 2 * chunk < n_tot ? 2 * chunk : n_tot;

  unsigned long long *bad;
  uint32_t *slot, *cnt;
  int *d_kmers;
  uint64_t *R;
  const bool to_out = (job.flags & PPK_FLAG_COUNTS) != 0;
  int rc = ppk_scratch_carve(dev, SLOT_PAIRS, [&](Carve &c) {
    c.take(bad, 1).take(slot, n_tot + 1).take(d_kmers, nk).take(cnt, to_out ? 1 : chunk * nk).take(R, img_rows * cols);
  });
  if (rc != PPK_OK) return rc;

  // -- the ids, before anything is read through one
  ppk_prof_stage("pairs_check", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  hipLaunchKernelGGL(pairs_validate_kernel, dim3(grid_for(m, 256 * 4, 4096)), dim3(256), 0, s, g, m, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  rc = ppk_read_back(dev, s, {{bad, 8}}, &h);
  ppk_prof_stage(nullptr, s);
  if (rc != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    long long i = 0, j = 0;
    if (!ppk_read_edge(job.d_i, job.d_j, job.stride, nullptr, (size_t)h[0], &i, &j, nullptr))
      return ppk_fail(PPK_ERR_HIP, "cannot read back the bad pair");
    const long long a = (i < j ? i : j) - job.int_offset, b = (i < j ? j : i) - job.int_offset;
    std::string why;
    if (!qry) why = a == b ? "a sample paired with itself" : "sample id out of range [0, " + std::to_string(n_ref) + ")";
    else if (a < 0 || (size_t)b >= n_tot) why = "id out of range [0, " + std::to_string(n_tot) + ")";
    else why = "both ids on one side (refs are [0, " + std::to_string(n_ref) + "), queries follow them)";
    return ppk_fail(PPK_ERR_ARG, "ppk_dist_pairs: pair " + std::to_string(h[0]) + " (i=" + std::to_string(i) + ", j=" +
                                     std::to_string(j) + "): " + why);
  }

  DistParams p = {};
  FitCoef coef = {};
  fit_params(ref, job.kmers, job.n_clu, job.flags, job.d_rtab, p, coef);
  p.self = qry ? 0 : 1;
  p.n_ref = n_ref;
  p.scale_x = p.scale_y = 1.0f;
  const bool use_clu = p.random_correct && p.n_clu > 1;
  const uint16_t *rclu = use_clu ? ref->d_clu : nullptr, *qclu = use_clu ? (qry ? qry : ref)->d_clu : nullptr;
  const float *rtab = p.random_correct ? job.d_rtab : nullptr;
  // the route of the rows: raw counts, Jaccard, the generic regression (what the dense route gives such a database)
  // or the table fit
  const bool jaccard = !to_out && (job.flags & PPK_FLAG_JACCARD), unfused = !to_out && !jaccard && ppk_unfused(ref);
  const bool packed = !to_out && !jaccard && !unfused;
  if (unfused) PPK_HIP(hipMemcpyAsync(d_kmers, job.kmers, nk * 4, hipMemcpyHostToDevice, s));
  if (packed && !job.lut_ready)
    if ((rc = enqueue_lut(ref, job.d_lut, job.d_rtab, p, coef, s)) != PPK_OK) return rc;

  // lanes per pair: the least power of two that holds a k's 64-bin blocks, at most a wave
  int G = 1;
  while (G < 64 && (size_t)G < ref->s64) G *= 2;
  const size_t ppw = 64 / G;
  const size_t out_row = (job.flags & (PPK_FLAG_COUNTS | PPK_FLAG_JACCARD)) ? nk * 4 : 8;
  for (size_t p0 = 0; p0 < m; p0 += chunk) {
    const size_t n = p0 + chunk < m ? chunk : m - p0;
    ppk_prof_stage("pairs_image", s);
    PPK_HIP(hipMemsetAsync(slot, 0xff, (n_tot + 1) * 4, s));
    hipLaunchKernelGGL(pairs_mark_kernel, dim3(grid_for(2 * n, 256 * 2, 4096)), dim3(256), 0, s, g, p0, n, slot, n_tot);
    hipLaunchKernelGGL(pairs_gather_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((n_ref + 31) / 32)), dim3(256),
                       0, s, ref->d_skT, n_ref, ref->npad, slot, R, cols, (int)ref->s64, (int)ref->bbits);
    if (qry)
      hipLaunchKernelGGL(pairs_gather_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((n_qry + 31) / 32)),
                         dim3(256), 0, s, qry->d_skT, n_qry, qry->npad, slot + n_ref, R, cols, (int)ref->s64,
                         (int)ref->bbits);
    PPK_HIP(hipGetLastError());

    ppk_prof_stage("pairs_counts", s);
    // a wave's span of the list: whole groups of pairs, about 16 of them while that leaves the device enough waves
    size_t waves = (n + ppw * 16 - 1) / (ppw * 16);
    const size_t min_waves = (size_t)ppk_geometry(dev).cus * 16;
    if (waves < min_waves) waves = (n + ppw - 1) / ppw < min_waves ? (n + ppw - 1) / ppw : min_waves;
    const size_t span = ((n + waves - 1) / waves + ppw - 1) / ppw * ppw;
    const size_t blocks = ((n + span - 1) / span + 3) / 4;
    uint32_t *c_out = to_out ? static_cast<uint32_t *>(job.d_out) + p0 * nk : cnt;
    hipLaunchKernelGGL(pairs_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, R, cols, slot, g, p0, n, span, G,
                       (int)nk, (int)ref->s64, (int)ref->bbits, c_out, packed ? n : (size_t)1, packed ? (size_t)1 : nk);
    PPK_HIP(hipGetLastError());

    if (!to_out) {
      ppk_prof_stage("pairs_fit", s);
      void *o = static_cast<char *>(job.d_out) + p0 * out_row;
      const dim3 grid((unsigned)((n + 255) / 256)), block(256);
      if (packed)
        hipLaunchKernelGGL(pairs_fit_kernel<0>, grid, block, 0, s, cnt, n, g, p0, job.d_lut, rclu, qclu, rtab, d_kmers, o,
                           job.d_n_failed, p);
      else if (unfused)
        hipLaunchKernelGGL(pairs_fit_kernel<1>, grid, block, 0, s, cnt, n, g, p0, job.d_lut, rclu, qclu, rtab, d_kmers, o,
                           job.d_n_failed, p);
      else
        hipLaunchKernelGGL(pairs_fit_kernel<2>, grid, block, 0, s, cnt, n, g, p0, job.d_lut, rclu, qclu, rtab, d_kmers, o,
                           job.d_n_failed, p);
      PPK_HIP(hipGetLastError());
    }
  }
  ppk_prof_stage(nullptr, s);
  return PPK_OK;
}

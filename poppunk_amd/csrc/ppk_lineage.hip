// Lineages within every strain from one pass over the resident long-form matrix.
//
// poppunk_lineages --create-db (PopPUNK/lineages.py:156-326) fits a LineageFit inside every strain: get_kNN_distances
// at a search depth that is, by the script's default, every other member of the strain, then lowerRank per rank.  Per
// strain that is a prune, a long -> square transform, a selection and a walk; here every strain is taken in one call.
//
//  - ppk_strain_knn_dev : every member's row of its strain, gathered from the long form (element (a, b), a < b, of the
//    condensed triangle), as 64-bit keys ord_of(distance) << 32 | local column, sorted ascending: get_kNN_distances'
//    stable order.  Three routes, chosen on the host per strain from its row length L = n_s - 1 (the segment offsets are
//    a host array, so every output offset is known before anything is launched):
//      wave   L <= 64: one wave per member, one key per lane, a bitonic network through the cross-lane shuffles; four
//             members per workgroup.  The refine boundary's strains are mostly this short.
//      lds    L <= 4 096 (option "lineage_lds_keys" lowers it): one workgroup per member, the keys in 32 KiB of LDS
//             (five workgroups per CU), a bitonic network over the next power of two.
//      long   longer rows: rocPRIM's segmented radix sort over scratch, a strain at a time in bands of rows that keep
//             both key buffers under option "lineage_scratch_mb".
//    A row is scattered in the long form whatever the route: the member lists are in the caller's order, not ascending,
//    so neither the contiguous stretch (columns above the member) nor the strided one (columns below) survives the
//    indirection through d_members; every lane computes the element of its own column.  Keys are unique (the column
//    breaks ties), so the three routes give the same bits.
//  - ppk_strain_ranks_dev : lowerRank's walk (src/extend.cpp:156-186, as ppk_sparse.hip's lr_walk_kernel states it) over
//    the sorted rows, once for all ranks: the walk's state does not depend on the rank, so rank q's row is the prefix
//    that ends where the walk would have stopped for it.  Then the level stream: one wave per row looks every kept
//    entry's mirror up by bisection in the other member's sorted row (the same long-form element, so the same key).
//    Compare and integer arithmetic only.
//  - ppk_strain_extend_dev : poppunk_refine.extend (src/extend.cpp:52-126, as ppk_sparse.hip states it) inside every
//    strain at once: a query batch merged into the stored lists from the resident query x reference
//    and query x query matrices.  A row's candidates get keys ord_of(distance) << 32 | side bit | place in the side's
//    list, which states the merge's order (query side first on a tie) and is unique, so the same three routes, chosen by
//    the rows of the extended strain, sort it; the output is ppk_strain_knn_dev's layout for the extended strains.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <string>
#include <vector>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaveKeys = 64;          // the wave route's longest row
constexpr int kLdsKeys = 4096;         // the LDS route's longest row: 32 KiB of keys
constexpr size_t kSortItems = (size_t)1 << 31;      // keys one segmented sort is given at most
constexpr int kMaxRanks = 1023;
constexpr uint64_t kNone = ~0ull;

// what the kernels of ppk_strain_knn_dev read
struct KnnArgs {
  const float *dist;           // [n(n-1)/2][2]
  size_t n;
  int col;
  const long long *members;    // [m]
  const long long *seg_off;    // [S + 1] (device copy)
  const long long *out_off;    // [S + 1]: entries of the output before strain s
  size_t depth;
  long long *oi, *oj;
  float *od;
};

__device__ __forceinline__ size_t lin_depth(size_t depth, size_t n_s) { return depth < n_s - 1 ? depth : n_s - 1; }

// the key of local column c in the row of the member with global id a (a != the id of c: ids are distinct)
__device__ __forceinline__ uint64_t lin_key(const KnnArgs &A, long long a, long long seg0, unsigned c) {
  const long long b = A.members[seg0 + c];
  const size_t lo = (size_t)(a < b ? a : b), hi = (size_t)(a < b ? b : a);
  const size_t e = lo * (2 * A.n - lo - 1) / 2 + (hi - lo - 1);
  return ((uint64_t)ord_of(A.dist[e * 2 + (size_t)A.col]) << 32) | (uint64_t)c;
}

// route row t of a route's list -> (strain, local row): rows[k] = the rows of the list's strains before strain k
__device__ __forceinline__ void lin_route_row(const int32_t *strains, const long long *rows, int n_list, long long t,
                                              int *s, long long *r) {
  int lo = 0, hi = n_list;             // the last k with rows[k] <= t
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (rows[mid] <= t) lo = mid;
    else hi = mid;
  }
  *s = strains[lo];
  *r = t - rows[lo];
}

__device__ __forceinline__ void lin_store(const KnnArgs &A, size_t at, long long r, uint64_t key) {
  A.oi[at] = r;
  A.oj[at] = (long long)(key & 0xffffffffull);
  A.od[at] = ord_inv((unsigned)(key >> 32));
}

// the 64 keys of a wave, one a lane, ascending: a bitonic network through the cross-lane shuffles
__device__ __forceinline__ uint64_t lin_wave_sort(uint64_t key, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint64_t other = __shfl_xor(key, j);
      const bool lower = (lane & j) == 0, up = (lane & k) == 0 || k == 64;
      const bool smaller = other < key;
      key = (lower == up) == smaller ? other : key;      // the lower lane of an ascending pair keeps the minimum
    }
  }
  return key;
}

// the `width` (a power of two) keys a workgroup holds in LDS, ascending; the keys are written and a barrier has passed
__device__ __forceinline__ void lin_lds_sort(uint64_t *s_keys, int width) {
  for (int k = 2; k <= width; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < width / 2; t += kThreads) {
        const int x = 2 * t - (t & (j - 1)), y = x + j;      // the pair (x, x + j), x without bit j
        const uint64_t u = s_keys[x], v = s_keys[y];
        const bool up = (x & k) == 0 || k == width;
        if ((u > v) == up) {
          s_keys[x] = v;
          s_keys[y] = u;
        }
      }
      __syncthreads();
    }
}

// wave route: grid = ceil(rows / 4)
__global__ void __launch_bounds__(kThreads) lin_wave_kernel(KnnArgs A, const int32_t *strains, const long long *rows,
                                                            int n_list, long long total) {
  const long long t = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= total) return;              // (wave-uniform; the kernel has no workgroup barrier)
  const int lane = threadIdx.x & 63;
  int s;
  long long r;
  lin_route_row(strains, rows, n_list, t, &s, &r);
  const long long seg0 = A.seg_off[s];
  const size_t n_s = (size_t)(A.seg_off[s + 1] - seg0);
  const int len = (int)(n_s - 1);      // <= 64
  uint64_t key = kNone;
  if (lane < len) key = lin_key(A, A.members[seg0 + r], seg0, (unsigned)(lane < r ? lane : lane + 1));
  key = lin_wave_sort(key, lane);
  const size_t d_s = lin_depth(A.depth, n_s);
  if ((size_t)lane < d_s) lin_store(A, (size_t)A.out_off[s] + (size_t)r * d_s + (size_t)lane, r, key);
}

// LDS route: one workgroup per row
__global__ void __launch_bounds__(kThreads) lin_lds_kernel(KnnArgs A, const int32_t *strains, const long long *rows,
                                                           int n_list) {
  __shared__ uint64_t s_keys[kLdsKeys];
  int s;
  long long r;
  lin_route_row(strains, rows, n_list, (long long)blockIdx.x, &s, &r);
  const long long seg0 = A.seg_off[s];
  const size_t n_s = (size_t)(A.seg_off[s + 1] - seg0);
  const int len = (int)(n_s - 1);      // <= kLdsKeys (the host's routing)
  int width = 2;
  while (width < len) width <<= 1;     // <= kLdsKeys
  const long long a = A.members[seg0 + r];
  for (int t = threadIdx.x; t < width; t += kThreads)
    s_keys[t] = t < len ? lin_key(A, a, seg0, (unsigned)(t < r ? t : t + 1)) : kNone;
  __syncthreads();
  lin_lds_sort(s_keys, width);
  const size_t d_s = lin_depth(A.depth, n_s);
  const size_t base = (size_t)A.out_off[s] + (size_t)r * d_s;
  for (size_t t = threadIdx.x; t < d_s; t += kThreads) lin_store(A, base + t, r, s_keys[t]);
}

// long route, one band: rows [r0, r0 + band) of strain s; keys[(r - r0) * len + slot]
__global__ void __launch_bounds__(kThreads) lin_fill_kernel(KnnArgs A, int s, long long r0, size_t items,
                                                            uint64_t *keys) {
  const long long seg0 = A.seg_off[s];
  const size_t len = (size_t)(A.seg_off[s + 1] - seg0) - 1;
  for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < items; t += (size_t)gridDim.x * kThreads) {
    const long long r = r0 + (long long)(t / len);
    const size_t slot = t % len;
    keys[t] = lin_key(A, A.members[seg0 + r], seg0, (unsigned)((long long)slot < r ? slot : slot + 1));
  }
}
__global__ void __launch_bounds__(kThreads) lin_emit_kernel(KnnArgs A, int s, long long r0, size_t rows,
                                                            const uint64_t *sorted) {
  const long long seg0 = A.seg_off[s];
  const size_t n_s = (size_t)(A.seg_off[s + 1] - seg0), len = n_s - 1, d_s = lin_depth(A.depth, n_s);
  const size_t items = rows * d_s;
  for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < items; t += (size_t)gridDim.x * kThreads) {
    const size_t row = t / d_s, pos = t % d_s;
    const long long r = r0 + (long long)row;
    lin_store(A, (size_t)A.out_off[s] + (size_t)r * d_s + pos, r, sorted[row * len + pos]);
  }
}
struct TimesLen {
  unsigned len;
  __host__ __device__ unsigned operator()(unsigned k) const { return k * len; }
};

// ---- validation of the member lists: owner[id] = the first position that holds id ------------------------------
__global__ void __launch_bounds__(kThreads) lin_owner_kernel(const long long *members, size_t m, size_t n,
                                                             int32_t *owner, unsigned long long *bad) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= m) return;
  const long long id = members[g];
  if (id < 0 || (size_t)id >= n) atomicMin(&bad[0], (unsigned long long)g);
  else atomicMin(&owner[id], (int32_t)g);
}
__global__ void __launch_bounds__(kThreads) lin_twice_kernel(const long long *members, size_t m, size_t n,
                                                             const int32_t *owner, unsigned long long *bad) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= m) return;
  const long long id = members[g];
  if (id >= 0 && (size_t)id < n && owner[id] != (int32_t)g) atomicMin(&bad[1], (unsigned long long)g);
}

// the strain that holds position g of the concatenated lists
size_t strain_of(const long long *seg_off, size_t n_strains, size_t g) {
  size_t lo = 0, hi = n_strains;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) / 2;
    if ((size_t)seg_off[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the segment errors that need no device; *m: the members of all strains
int lin_check_segments(const std::string &who, const long long *seg_off, size_t n_strains, size_t *m) {
  if (!seg_off) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (n_strains == 0 || n_strains >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n_strains must be 1 .. 2^31 - 2");
  if (seg_off[0] != 0) return ppk_fail(PPK_ERR_ARG, who + ": seg_off[0] must be 0");
  for (size_t s = 0; s < n_strains; ++s) {
    const long long len = seg_off[s + 1] - seg_off[s];
    if (len < 2)
      return ppk_fail(PPK_ERR_ARG, who + ": strain " + std::to_string(s) + " has " + std::to_string(len) +
                                       " members: a strain needs at least 2");
  }
  if (seg_off[n_strains] > 0x7f000000ll) return ppk_fail(PPK_ERR_ARG, who + ": fewer than 2^31 - 2^24 members supported");
  *m = (size_t)seg_off[n_strains];
  return PPK_OK;
}

// ---- ranks ----------------------------------------------------------------------------------------------------
struct RankArgs {
  const long long *j;          // the sorted lists: local column, distance
  const float *d;
  const long long *seg_off, *out_off;      // device copies
  const int32_t *ranks;        // [R] ascending
  int n_strains, n_ranks;
  size_t m, depth;
  int reciprocal, count_unique;
  float epsilon;
  int32_t *prefix;             // [R][m]
};

__device__ __forceinline__ int lin_strain_of(const long long *seg_off, int n_strains, long long g) {
  int lo = 0, hi = n_strains;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (seg_off[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// lowerRank's walk over a sorted row (src/extend.cpp:156-186), once for every rank: rank q's prefix ends where
// `unique` first passes ranks[q].  A column outside the strain, or the row itself, raises bad[0] (the row's position).
__global__ void __launch_bounds__(kThreads) lin_prefix_kernel(RankArgs A, unsigned long long *bad) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= A.m) return;
  const int s = lin_strain_of(A.seg_off, A.n_strains, (long long)g);
  const long long seg0 = A.seg_off[s];
  const size_t n_s = (size_t)(A.seg_off[s + 1] - seg0), d_s = lin_depth(A.depth, n_s);
  const long long r = (long long)g - seg0;
  const size_t base = (size_t)A.out_off[s] + (size_t)r * d_s;
  unsigned long long kept = 0, unique = 0;
  float prev = 0.0f;
  int q = 0;
  for (size_t e = 0; e < d_s && q < A.n_ranks; ++e) {
    const long long j = A.j[base + e];
    if (j < 0 || (size_t)j >= n_s || j == r) {      // (ppk_strain_knn_dev's lists never hold the row itself)
      atomicMin(&bad[0], (unsigned long long)g);
      break;
    }
    if (A.count_unique) {
      const float dist = A.d[base + e];
      if (fabsf(__fsub_rn(dist, prev)) >= A.epsilon) {
        ++unique;
        prev = dist;
      }
    } else {
      unique = kept;
    }
    while (q < A.n_ranks && unique > (unsigned long long)A.ranks[q]) A.prefix[(size_t)q++ * A.m + g] = (int32_t)kept;
    if (q < A.n_ranks) ++kept;
  }
  // (the ranks the row ran out under keep all of it)
  while (q < A.n_ranks) A.prefix[(size_t)q++ * A.m + g] = (int32_t)kept;
}

// the lowest rank index whose prefix of row g holds place p (p < the last rank's prefix)
__device__ __forceinline__ int lin_level(const RankArgs &A, size_t g, int p) {
  int q = 0;
  while (q < A.n_ranks - 1 && p >= A.prefix[(size_t)q * A.m + g]) ++q;
  return q;
}

// One wave per row g.  Every entry (r -> c) at place p the last rank keeps looks its mirror (c -> r) up in the kept part
// of c's sorted row: the same matrix element, so the same distance, found by bisection on the key of the distance and a
// scan of the run of equal keys for the column (a run of length L costs up to L reads; inside a run the order is by
// column in ppk_strain_knn_dev's lists and query side first in ppk_strain_extend_dev's).  An unordered pair goes out once: where both directions are kept, from the lower row, at the earlier of the
// two levels (reciprocal_only: the later); where one is, from that row at its level (reciprocal_only: not at all).
template <bool WRITE>
__global__ void __launch_bounds__(kThreads) lin_stream_kernel(RankArgs A, unsigned long long *count,
                                                              const unsigned long long *offs, long long *pos_i,
                                                              long long *pos_j, long long *level, float *sdist) {
  const size_t g = (size_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (g >= A.m) return;                // (wave-uniform; no workgroup barrier)
  const int lane = threadIdx.x & 63;
  const int s = lin_strain_of(A.seg_off, A.n_strains, (long long)g);
  const long long seg0 = A.seg_off[s];
  const size_t n_s = (size_t)(A.seg_off[s + 1] - seg0), d_s = lin_depth(A.depth, n_s);
  const long long r = (long long)g - seg0;
  const size_t strain_base = (size_t)A.out_off[s], base = strain_base + (size_t)r * d_s;
  const int32_t *last = A.prefix + (size_t)(A.n_ranks - 1) * A.m;
  const int kept = last[g];
  unsigned long long at = WRITE ? offs[g] : 0, total = 0;
  for (int p0 = 0; p0 < kept; p0 += 64) {
    const int p = p0 + lane;
    bool emit = false;
    long long c = 0;
    float dist = 0.0f;
    int lv = 0;
    if (p < kept) {
      c = A.j[base + p];
      dist = A.d[base + p];
      if (c >= 0 && (size_t)c < n_s && c != r) {      // (anything else has raised bad[0] in the walk)
        lv = lin_level(A, g, p);
        const size_t g2 = (size_t)(seg0 + c), base2 = strain_base + (size_t)c * d_s;
        const unsigned key = ord_of(dist);
        int lo = 0, hi = last[g2];                    // the first place of c's kept part whose key is not below `key`
        while (lo < hi) {
          const int mid = (lo + hi) / 2;
          if (ord_of(A.d[base2 + mid]) < key) lo = mid + 1;
          else hi = mid;
        }
        // the run of equal distances is scanned for the column: ppk_strain_knn_dev orders it by column, extend does not
        bool both = false;
        for (; !both && lo < last[g2] && ord_of(A.d[base2 + lo]) == key; ++lo) both = A.j[base2 + lo] == r;
        lo -= both;
        if (both) {
          const int lv2 = lin_level(A, g2, lo);
          emit = r < c;
          lv = A.reciprocal ? (lv2 > lv ? lv2 : lv) : (lv2 < lv ? lv2 : lv);
        } else {
          emit = !A.reciprocal;
        }
      }
    }
    const unsigned long long mask = __ballot(emit);
    if (WRITE && emit) {
      const unsigned long long o = at + total + __popcll(mask & ((1ull << lane) - 1));
      pos_i[o] = (long long)g;
      pos_j[o] = seg0 + c;
      level[o] = lv;
      if (sdist) sdist[o] = dist;
    }
    total += __popcll(mask);
  }
  if (!WRITE && lane == 0) count[g] = total;
}

// ---- extend ---------------------------------------------------------------------------------------------------
// what the kernels of ppk_strain_extend_dev read
struct ExtArgs {
  const float *qr, *qq;        // [n_qry * n_ref][2] query-major; [n_qry(n_qry-1)/2][2] long form
  size_t n_ref, n_qry;
  int col;
  float floor;
  const long long *members, *queries;      // [m], [mq]
  const long long *seg_off, *qry_off;      // [S + 1] (device copies)
  const long long *nn_off, *out_off;       // [S + 1]: entries of the stored lists / of the output before strain s
  const long long *nn_j;       // the stored lists
  const float *nn_d;
  size_t depth;
  long long *oi, *oj;
  float *od;
};

constexpr uint64_t kStoredSide = 0x80000000ull;      // bit 31 of a key: the stored side, after the query side on a tie

__device__ __forceinline__ float ext_floor(const ExtArgs &A, float v) { return v < A.floor ? A.floor : v; }

// Candidate `slot` of local row r of strain s, as ord_of(distance) << 32 | side | place in the side's list.  A row has
// n_s + q_s - 1 slots: the query side first (a reference row: the q_s queries; a query row: the others), then the
// stored side (a reference row: its stored row, and kNone for what is left; a query row: the n_s members).
__device__ __forceinline__ uint64_t ext_key(const ExtArgs &A, int s, long long r, size_t slot) {
  const long long seg0 = A.seg_off[s], q0 = A.qry_off[s];
  const size_t n_s = (size_t)(A.seg_off[s + 1] - seg0), q_s = (size_t)(A.qry_off[s + 1] - q0);
  if ((size_t)r < n_s) {
    if (slot < q_s) {
      const size_t e = (size_t)A.queries[q0 + (long long)slot] * A.n_ref + (size_t)A.members[seg0 + r];
      return ((uint64_t)ord_of(ext_floor(A, A.qr[e * 2 + (size_t)A.col])) << 32) | (uint64_t)slot;
    }
    const size_t p = slot - q_s, d_s = lin_depth(A.depth, n_s);
    if (p >= d_s) return kNone;
    return ((uint64_t)ord_of(A.nn_d[(size_t)A.nn_off[s] + (size_t)r * d_s + p]) << 32) | kStoredSide | (uint64_t)p;
  }
  const size_t k0 = (size_t)r - n_s;
  const size_t a = (size_t)A.queries[q0 + (long long)k0];
  if (slot + 1 < q_s) {
    const size_t k = slot < k0 ? slot : slot + 1;
    const size_t b = (size_t)A.queries[q0 + (long long)k];
    const size_t lo = a < b ? a : b, hi = a < b ? b : a;
    const size_t e = lo * (2 * A.n_qry - lo - 1) / 2 + (hi - lo - 1);
    return ((uint64_t)ord_of(ext_floor(A, A.qq[e * 2 + (size_t)A.col])) << 32) | (uint64_t)k;
  }
  const size_t c = slot + 1 - q_s;     // < n_s
  const size_t e = a * A.n_ref + (size_t)A.members[seg0 + (long long)c];
  return ((uint64_t)ord_of(ext_floor(A, A.qr[e * 2 + (size_t)A.col])) << 32) | kStoredSide | (uint64_t)c;
}

// entry `pos` of the output row r of strain s from its sorted key
__device__ __forceinline__ void ext_store(const ExtArgs &A, int s, long long r, size_t pos, uint64_t key) {
  const size_t n_s = (size_t)(A.seg_off[s + 1] - A.seg_off[s]), q_s = (size_t)(A.qry_off[s + 1] - A.qry_off[s]);
  const size_t d_out = lin_depth(A.depth, n_s + q_s), at = (size_t)A.out_off[s] + (size_t)r * d_out + pos;
  const size_t place = (size_t)(key & 0x7fffffffull);
  long long col;
  if (!(key & kStoredSide)) col = (long long)(n_s + place);
  else if ((size_t)r < n_s) col = A.nn_j[(size_t)A.nn_off[s] + (size_t)r * lin_depth(A.depth, n_s) + place];
  else col = (long long)place;
  A.oi[at] = r;
  A.oj[at] = col;
  A.od[at] = ord_inv((unsigned)(key >> 32));
}

__device__ __forceinline__ size_t ext_rows(const ExtArgs &A, int s) {
  return (size_t)(A.seg_off[s + 1] - A.seg_off[s]) + (size_t)(A.qry_off[s + 1] - A.qry_off[s]);
}

// the three routes of ppk_strain_knn_dev over the rows of the extended strains (rows[k]: extended rows before strain k
// of the route's list); a row's n'_s - 1 slots are sorted whole, so the merge needs no separate statement
__global__ void __launch_bounds__(kThreads) ext_wave_kernel(ExtArgs A, const int32_t *strains, const long long *rows,
                                                            int n_list, long long total) {
  const long long t = (long long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (t >= total) return;              // (wave-uniform; the kernel has no workgroup barrier)
  const int lane = threadIdx.x & 63;
  int s;
  long long r;
  lin_route_row(strains, rows, n_list, t, &s, &r);
  const size_t n_x = ext_rows(A, s);
  uint64_t key = kNone;
  if ((size_t)lane < n_x - 1) key = ext_key(A, s, r, (size_t)lane);
  key = lin_wave_sort(key, lane);
  if ((size_t)lane < lin_depth(A.depth, n_x)) ext_store(A, s, r, (size_t)lane, key);
}

__global__ void __launch_bounds__(kThreads) ext_lds_kernel(ExtArgs A, const int32_t *strains, const long long *rows,
                                                           int n_list) {
  __shared__ uint64_t s_keys[kLdsKeys];
  int s;
  long long r;
  lin_route_row(strains, rows, n_list, (long long)blockIdx.x, &s, &r);
  const size_t n_x = ext_rows(A, s);
  const int len = (int)(n_x - 1);      // <= kLdsKeys (the host's routing)
  int width = 2;
  while (width < len) width <<= 1;
  for (int t = threadIdx.x; t < width; t += kThreads) s_keys[t] = t < len ? ext_key(A, s, r, (size_t)t) : kNone;
  __syncthreads();
  lin_lds_sort(s_keys, width);
  const size_t d_out = lin_depth(A.depth, n_x);
  for (size_t t = threadIdx.x; t < d_out; t += kThreads) ext_store(A, s, r, t, s_keys[t]);
}

// long route, one band: rows [r0, r0 + band) of strain s; keys[(r - r0) * len + slot], len = n'_s - 1
__global__ void __launch_bounds__(kThreads) ext_fill_kernel(ExtArgs A, int s, long long r0, size_t items, size_t len,
                                                            uint64_t *keys) {
  for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < items; t += (size_t)gridDim.x * kThreads)
    keys[t] = ext_key(A, s, r0 + (long long)(t / len), t % len);
}
__global__ void __launch_bounds__(kThreads) ext_emit_kernel(ExtArgs A, int s, long long r0, size_t rows, size_t len,
                                                            const uint64_t *sorted) {
  const size_t d_out = lin_depth(A.depth, len + 1), items = rows * d_out;
  for (size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x; t < items; t += (size_t)gridDim.x * kThreads) {
    const size_t row = t / d_out, pos = t % d_out;
    ext_store(A, s, r0 + (long long)row, pos, sorted[row * len + pos]);
  }
}

// the stored lists, an entry a thread: bad[0] = the first entry whose column leaves its strain or is its row, or whose
// distance is below the entry before it in the row
__global__ void __launch_bounds__(kThreads) ext_stored_kernel(const long long *nn_j, const float *nn_d,
                                                              const long long *seg_off, const long long *nn_off,
                                                              int n_strains, size_t depth, size_t nnz,
                                                              unsigned long long *bad) {
  const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= nnz) return;
  const int s = lin_strain_of(nn_off, n_strains, (long long)e);
  const size_t n_s = (size_t)(seg_off[s + 1] - seg_off[s]), d_s = lin_depth(depth, n_s);
  const size_t in = e - (size_t)nn_off[s], r = in / d_s, p = in % d_s;
  const long long j = nn_j[e];
  if (j < 0 || (size_t)j >= n_s || (size_t)j == r || (p > 0 && ord_of(nn_d[e]) < ord_of(nn_d[e - 1])))
    atomicMin(&bad[0], (unsigned long long)e);
}

// the offsets of the sorted lists: out_off[s] = the entries of the strains before s
std::vector<long long> lin_out_offsets(const long long *seg_off, size_t n_strains, size_t depth) {
  std::vector<long long> out(n_strains + 1, 0);
  for (size_t s = 0; s < n_strains; ++s) {
    const size_t n_s = (size_t)(seg_off[s + 1] - seg_off[s]);
    out[s + 1] = out[s] + (long long)(n_s * (depth < n_s - 1 ? depth : n_s - 1));
  }
  return out;
}

// The routes of a call over segments of n rows of n - 1 keys each (ppk_strain_knn_dev: the strains; ppk_strain_extend_dev:
// the extended strains), chosen on the host: the wave and LDS routes' segments with the rows before each, the long
// route's bands; then their device copies and the long route's buffers, taken inside the call's one carve.
struct LinRoutes {
  struct Band {
    int s;
    long long r0;
    size_t rows, len;
  };
  std::vector<int32_t> wave_s, lds_s;
  std::vector<long long> wave_rows = std::vector<long long>(1, 0), lds_rows = std::vector<long long>(1, 0);
  std::vector<Band> bands;
  size_t most_keys = 0, tmp_bytes = 0;
  int32_t *d_wave_s = nullptr, *d_lds_s = nullptr;
  long long *d_wave_rows = nullptr, *d_lds_rows = nullptr;
  uint64_t *keys_in = nullptr, *keys_out = nullptr;
  char *tmp = nullptr;

  void take(Carve &c) {
    c.take(d_wave_s, wave_s.size()).take(d_wave_rows, wave_rows.size()).take(d_lds_s, lds_s.size());
    c.take(d_lds_rows, lds_rows.size()).take(keys_in, most_keys).take(keys_out, most_keys).take(tmp, tmp_bytes + 256);
  }
  int upload(hipStream_t s) const {
    if (!wave_s.empty()) {
      PPK_HIP(hipMemcpyAsync(d_wave_s, wave_s.data(), wave_s.size() * 4, hipMemcpyHostToDevice, s));
      PPK_HIP(hipMemcpyAsync(d_wave_rows, wave_rows.data(), wave_rows.size() * 8, hipMemcpyHostToDevice, s));
    }
    if (!lds_s.empty()) {
      PPK_HIP(hipMemcpyAsync(d_lds_s, lds_s.data(), lds_s.size() * 4, hipMemcpyHostToDevice, s));
      PPK_HIP(hipMemcpyAsync(d_lds_rows, lds_rows.data(), lds_rows.size() * 8, hipMemcpyHostToDevice, s));
    }
    return PPK_OK;
  }
  // the sort of one band's keys: keys_in -> keys_out
  int sort(const Band &b, hipStream_t s) const {
    size_t bytes = tmp_bytes;
    const auto begin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0), TimesLen{(unsigned)b.len});
    PPK_HIP(rocprim::segmented_radix_sort_keys(tmp, bytes, (const uint64_t *)keys_in, keys_out,
                                               (unsigned)(b.rows * b.len), (unsigned)b.rows, begin, begin + 1, 0u, 64u, s));
    return PPK_OK;
  }
};

int lin_route(const std::string &who, const long long *seg, size_t n_segs, hipStream_t s, LinRoutes *R) {
  long long lds_max = ppk_config().lineage_lds_keys.load();
  if (lds_max <= 0 || lds_max > kLdsKeys) lds_max = kLdsKeys;
  const long long cap_mb = ppk_config().lineage_scratch_mb.load();
  const size_t room = ((size_t)(cap_mb > 0 ? cap_mb : 0) << 20) / 5 * 4;      // (a slot is allocated with a quarter to spare)
  for (size_t t = 0; t < n_segs; ++t) {
    const size_t n_s = (size_t)(seg[t + 1] - seg[t]), len = n_s - 1;
    if (len <= (size_t)kWaveKeys) {
      R->wave_s.push_back((int32_t)t);
      R->wave_rows.push_back(R->wave_rows.back() + (long long)n_s);
    } else if (len <= (size_t)lds_max) {
      R->lds_s.push_back((int32_t)t);
      R->lds_rows.push_back(R->lds_rows.back() + (long long)n_s);
    } else {
      if (len >= kSortItems) return ppk_fail(PPK_ERR_ARG, who + ": a strain of 2^31 members or more");
      size_t rows = room / (len * 2 * sizeof(uint64_t));      // both key buffers of a band under the cap; at least a row
      if (rows > kSortItems / len) rows = kSortItems / len;
      if (rows < 1) rows = 1;
      if (rows > n_s) rows = n_s;
      for (size_t r0 = 0; r0 < n_s; r0 += rows) {
        const size_t take = r0 + rows < n_s ? rows : n_s - r0;
        R->bands.push_back(LinRoutes::Band{(int)t, (long long)r0, take, len});
      }
      if (rows * len > R->most_keys) R->most_keys = rows * len;
      size_t bytes = 0;
      const auto begin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0), TimesLen{(unsigned)len});
      PPK_HIP(rocprim::segmented_radix_sort_keys(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                 (unsigned)(rows * len), (unsigned)rows, begin, begin + 1, 0u, 64u, s));
      if (bytes > R->tmp_bytes) R->tmp_bytes = bytes;
    }
  }
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_strain_knn_dev(const float *d_dist, size_t n, int dist_col, const long long *d_members,
                                  const long long *seg_off, size_t n_strains, size_t depth, long long *d_i,
                                  long long *d_j, float *d_out, void *stream) {
  const std::string who = "ppk_strain_knn";
  if (!d_dist || !d_members || !d_i || !d_j || !d_out) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (dist_col != 0 && dist_col != 1) return ppk_fail(PPK_ERR_ARG, who + ": dist_col must be 0 or 1");
  if (n < 2 || n >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n must be 2 .. 2^31 - 2");
  if (depth == 0) return ppk_fail(PPK_ERR_ARG, who + ": depth must be at least 1");
  size_t m = 0;
  int rc = lin_check_segments(who, seg_off, n_strains, &m);
  if (rc != PPK_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);

  // routing, on the host
  const std::vector<long long> out_off = lin_out_offsets(seg_off, n_strains, depth);
  LinRoutes R;
  if ((rc = lin_route(who, seg_off, n_strains, s, &R)) != PPK_OK) return rc;

  KnnArgs A{};
  A.dist = d_dist;
  A.n = n;
  A.col = dist_col;
  A.members = d_members;
  A.depth = depth;
  A.oi = d_i;
  A.oj = d_j;
  A.od = d_out;
  unsigned long long *bad;
  int32_t *owner;
  long long *d_seg, *d_off;
  rc = ppk_scratch_carve(dev, SLOT_LINEAGE, [&](Carve &c) {
    c.take(bad, 2).take(owner, n).take(d_seg, n_strains + 1).take(d_off, n_strains + 1);
    R.take(c);
  });
  if (rc != PPK_OK) return rc;
  A.seg_off = d_seg;
  A.out_off = d_off;

  // the member lists, before anything indexes by them: the call's one synchronisation
  ppk_prof_stage("check", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 16, s));
  PPK_HIP(hipMemsetAsync(owner, 0x7f, n * sizeof(int32_t), s));
  PPK_HIP(hipMemcpyAsync(d_seg, seg_off, (n_strains + 1) * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_off, out_off.data(), (n_strains + 1) * 8, hipMemcpyHostToDevice, s));
  if ((rc = R.upload(s)) != PPK_OK) return rc;
  const unsigned m_grid = grid_for(m, kThreads, ~0u);
  hipLaunchKernelGGL(lin_owner_kernel, dim3(m_grid), dim3(kThreads), 0, s, d_members, m, n, owner, bad);
  hipLaunchKernelGGL(lin_twice_kernel, dim3(m_grid), dim3(kThreads), 0, s, d_members, m, n, owner, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  rc = ppk_read_back(dev, s, {{bad, 16}}, &h);
  ppk_prof_stage(nullptr, s);
  if (rc != PPK_OK) return rc;
  const unsigned long long first = h[0] < h[1] ? h[0] : h[1];
  if (first != ~0ull) {
    const bool range = h[0] <= h[1];
    const size_t g = (size_t)first, t = strain_of(seg_off, n_strains, g);
    long long id = 0;
    PPK_HIP(hipMemcpy(&id, d_members + g, 8, hipMemcpyDeviceToHost));
    const std::string where = who + ": strain " + std::to_string(t) + ", member " +
                              std::to_string(g - (size_t)seg_off[t]) + ": sample " + std::to_string(id);
    if (range) return ppk_fail(PPK_ERR_ARG, where + " outside [0, " + std::to_string(n) + ")");
    int32_t g0 = 0;
    PPK_HIP(hipMemcpy(&g0, owner + id, 4, hipMemcpyDeviceToHost));
    const size_t t0 = strain_of(seg_off, n_strains, (size_t)g0);
    return ppk_fail(PPK_ERR_ARG, where + " is already member " + std::to_string((size_t)g0 - (size_t)seg_off[t0]) +
                                     " of strain " + std::to_string(t0));
  }

  if (!R.wave_s.empty()) {
    ppk_prof_stage("wave", s);
    const long long total = R.wave_rows.back();
    hipLaunchKernelGGL(lin_wave_kernel, dim3(grid_for((size_t)total, kThreads / 64, ~0u)), dim3(kThreads), 0, s, A,
                       R.d_wave_s, R.d_wave_rows, (int)R.wave_s.size(), total);
  }
  if (!R.lds_s.empty()) {
    ppk_prof_stage("lds", s);
    hipLaunchKernelGGL(lin_lds_kernel, dim3((unsigned)R.lds_rows.back()), dim3(kThreads), 0, s, A, R.d_lds_s,
                       R.d_lds_rows, (int)R.lds_s.size());
  }
  PPK_HIP(hipGetLastError());
  if (!R.bands.empty()) ppk_prof_stage("long", s);
  for (const LinRoutes::Band &b : R.bands) {
    const size_t items = b.rows * b.len;
    hipLaunchKernelGGL(lin_fill_kernel, dim3(grid_for(items, kThreads * 4, 65536)), dim3(kThreads), 0, s, A, b.s, b.r0,
                       items, R.keys_in);
    if ((rc = R.sort(b, s)) != PPK_OK) return rc;
    hipLaunchKernelGGL(lin_emit_kernel, dim3(grid_for(items, kThreads * 4, 65536)), dim3(kThreads), 0, s, A, b.s, b.r0,
                       b.rows, R.keys_out);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

namespace {

// the query segments, and the segments of the extended strains (n'_s = n_s + q_s rows each)
int ext_check_queries(const std::string &who, const long long *seg_off, const long long *qry_off, size_t n_strains,
                      size_t *mq, std::vector<long long> *ext_seg) {
  if (!qry_off) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (qry_off[0] != 0) return ppk_fail(PPK_ERR_ARG, who + ": qry_off[0] must be 0");
  ext_seg->assign(n_strains + 1, 0);
  for (size_t s = 0; s < n_strains; ++s) {
    if (qry_off[s + 1] < qry_off[s])
      return ppk_fail(PPK_ERR_ARG, who + ": strain " + std::to_string(s) + " has a negative number of queries");
    (*ext_seg)[s + 1] = seg_off[s + 1] + qry_off[s + 1];
  }
  if ((*ext_seg)[n_strains] > 0x7f000000ll)
    return ppk_fail(PPK_ERR_ARG, who + ": fewer than 2^31 - 2^24 members and queries supported");
  *mq = (size_t)qry_off[n_strains];
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_strain_extend_dev(const long long *d_members, const long long *seg_off, const long long *d_queries,
                                     const long long *qry_off, size_t n_strains, const long long *d_nn_j,
                                     const float *d_nn_d, const float *d_qr, const float *d_qq, size_t n_ref,
                                     size_t n_qry, int dist_col, float floor, size_t depth, long long *d_i,
                                     long long *d_j, float *d_out, void *stream) {
  const std::string who = "ppk_strain_extend";
  if (!d_members || !d_nn_j || !d_nn_d || !d_i || !d_j || !d_out) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (dist_col != 0 && dist_col != 1) return ppk_fail(PPK_ERR_ARG, who + ": dist_col must be 0 or 1");
  if (n_ref < 2 || n_ref >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n_ref must be 2 .. 2^31 - 2");
  if (n_qry >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n_qry must be below 2^31 - 1");
  if (depth == 0) return ppk_fail(PPK_ERR_ARG, who + ": depth must be at least 1");
  size_t m = 0, mq = 0;
  int rc = lin_check_segments(who, seg_off, n_strains, &m);
  if (rc != PPK_OK) return rc;
  std::vector<long long> ext_seg;
  if ((rc = ext_check_queries(who, seg_off, qry_off, n_strains, &mq, &ext_seg)) != PPK_OK) return rc;
  if (mq && (!d_queries || !d_qr)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  for (size_t t = 0; t < n_strains && !d_qq; ++t)
    if (qry_off[t + 1] - qry_off[t] >= 2)
      return ppk_fail(PPK_ERR_ARG, who + ": strain " + std::to_string(t) + " has " +
                                       std::to_string(qry_off[t + 1] - qry_off[t]) + " queries and d_qq is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);

  // routing, on the host, as ppk_strain_knn_dev's: by the n'_s - 1 slots of a row of the extended strain
  const std::vector<long long> nn_off = lin_out_offsets(seg_off, n_strains, depth);
  const std::vector<long long> out_off = lin_out_offsets(ext_seg.data(), n_strains, depth);
  const size_t nnz = (size_t)nn_off.back();
  LinRoutes R;
  if ((rc = lin_route(who, ext_seg.data(), n_strains, s, &R)) != PPK_OK) return rc;

  ExtArgs A{};
  A.qr = d_qr;
  A.qq = d_qq;
  A.n_ref = n_ref;
  A.n_qry = n_qry;
  A.col = dist_col;
  A.floor = floor;
  A.members = d_members;
  A.queries = d_queries;
  A.nn_j = d_nn_j;
  A.nn_d = d_nn_d;
  A.depth = depth;
  A.oi = d_i;
  A.oj = d_j;
  A.od = d_out;
  unsigned long long *bad;
  int32_t *owner, *owner_q;
  long long *d_offs;
  const size_t S1 = n_strains + 1;
  rc = ppk_scratch_carve(dev, SLOT_LINEAGE, [&](Carve &c) {
    c.take(bad, 5).take(owner, n_ref).take(owner_q, n_qry ? n_qry : 1).take(d_offs, 4 * S1);
    R.take(c);
  });
  if (rc != PPK_OK) return rc;
  A.seg_off = d_offs;
  A.qry_off = d_offs + S1;
  A.nn_off = d_offs + 2 * S1;
  A.out_off = d_offs + 3 * S1;

  // both id lists and the stored lists, before anything indexes by them: the call's one synchronisation
  ppk_prof_stage("check", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 40, s));
  PPK_HIP(hipMemsetAsync(owner, 0x7f, n_ref * sizeof(int32_t), s));
  if (n_qry) PPK_HIP(hipMemsetAsync(owner_q, 0x7f, n_qry * sizeof(int32_t), s));
  PPK_HIP(hipMemcpyAsync(d_offs, seg_off, S1 * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_offs + S1, qry_off, S1 * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_offs + 2 * S1, nn_off.data(), S1 * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_offs + 3 * S1, out_off.data(), S1 * 8, hipMemcpyHostToDevice, s));
  if ((rc = R.upload(s)) != PPK_OK) return rc;
  const unsigned m_grid = grid_for(m, kThreads, ~0u), q_grid = grid_for(mq, kThreads, ~0u);
  hipLaunchKernelGGL(lin_owner_kernel, dim3(m_grid), dim3(kThreads), 0, s, d_members, m, n_ref, owner, bad);
  hipLaunchKernelGGL(lin_twice_kernel, dim3(m_grid), dim3(kThreads), 0, s, d_members, m, n_ref, owner, bad);
  if (mq) {
    hipLaunchKernelGGL(lin_owner_kernel, dim3(q_grid), dim3(kThreads), 0, s, d_queries, mq, n_qry, owner_q, bad + 2);
    hipLaunchKernelGGL(lin_twice_kernel, dim3(q_grid), dim3(kThreads), 0, s, d_queries, mq, n_qry, owner_q, bad + 2);
  }
  hipLaunchKernelGGL(ext_stored_kernel, dim3(grid_for(nnz, kThreads, ~0u)), dim3(kThreads), 0, s, d_nn_j, d_nn_d,
                     A.seg_off, A.nn_off, (int)n_strains, depth, nnz, bad + 4);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  rc = ppk_read_back(dev, s, {{bad, 40}}, &h);
  ppk_prof_stage(nullptr, s);
  if (rc != PPK_OK) return rc;
  // the first offender: the members, then the queries, then the stored lists
  for (int list = 0; list < 2; ++list) {
    const unsigned long long *w = h + 2 * list;
    const unsigned long long first = w[0] < w[1] ? w[0] : w[1];
    if (first == ~0ull) continue;
    const long long *off = list ? qry_off : seg_off, *d_ids = list ? d_queries : d_members;
    const std::string item = list ? "query" : "member", what = list ? "query" : "sample";
    const size_t g = (size_t)first, t = strain_of(off, n_strains, g), limit = list ? n_qry : n_ref;
    long long id = 0;
    PPK_HIP(hipMemcpy(&id, d_ids + g, 8, hipMemcpyDeviceToHost));
    const std::string where = who + ": strain " + std::to_string(t) + ", " + item + " " +
                              std::to_string(g - (size_t)off[t]) + ": " + what + " " + std::to_string(id);
    if (w[0] <= w[1]) return ppk_fail(PPK_ERR_ARG, where + " outside [0, " + std::to_string(limit) + ")");
    int32_t g0 = 0;
    PPK_HIP(hipMemcpy(&g0, (list ? owner_q : owner) + id, 4, hipMemcpyDeviceToHost));
    const size_t t0 = strain_of(off, n_strains, (size_t)g0);
    return ppk_fail(PPK_ERR_ARG, where + " is already " + item + " " + std::to_string((size_t)g0 - (size_t)off[t0]) +
                                     " of strain " + std::to_string(t0));
  }
  if (h[4] != ~0ull) {
    const size_t e = (size_t)h[4], t = strain_of(nn_off.data(), n_strains, e);
    const size_t n_s = (size_t)(seg_off[t + 1] - seg_off[t]), d_s = depth < n_s - 1 ? depth : n_s - 1;
    const size_t in = e - (size_t)nn_off[t], r = in / d_s, p = in % d_s;
    long long col = 0;
    PPK_HIP(hipMemcpy(&col, d_nn_j + e, 8, hipMemcpyDeviceToHost));
    const std::string where = who + ": strain " + std::to_string(t) + ", row " + std::to_string(r) + ", entry " +
                              std::to_string(p) + ": ";
    if (col < 0 || (size_t)col >= n_s)
      return ppk_fail(PPK_ERR_ARG, where + "column " + std::to_string(col) + " outside [0, " + std::to_string(n_s) + ")");
    if ((size_t)col == r) return ppk_fail(PPK_ERR_ARG, where + "column " + std::to_string(col) + " is the row itself");
    return ppk_fail(PPK_ERR_ARG, where + "the distance is below the entry before it");
  }

  if (!R.wave_s.empty()) {
    ppk_prof_stage("wave", s);
    const long long total = R.wave_rows.back();
    hipLaunchKernelGGL(ext_wave_kernel, dim3(grid_for((size_t)total, kThreads / 64, ~0u)), dim3(kThreads), 0, s, A,
                       R.d_wave_s, R.d_wave_rows, (int)R.wave_s.size(), total);
  }
  if (!R.lds_s.empty()) {
    ppk_prof_stage("lds", s);
    hipLaunchKernelGGL(ext_lds_kernel, dim3((unsigned)R.lds_rows.back()), dim3(kThreads), 0, s, A, R.d_lds_s,
                       R.d_lds_rows, (int)R.lds_s.size());
  }
  PPK_HIP(hipGetLastError());
  if (!R.bands.empty()) ppk_prof_stage("long", s);
  for (const LinRoutes::Band &b : R.bands) {
    const size_t items = b.rows * b.len;
    hipLaunchKernelGGL(ext_fill_kernel, dim3(grid_for(items, kThreads * 4, 65536)), dim3(kThreads), 0, s, A, b.s, b.r0,
                       items, b.len, R.keys_in);
    if ((rc = R.sort(b, s)) != PPK_OK) return rc;
    hipLaunchKernelGGL(ext_emit_kernel, dim3(grid_for(items, kThreads * 4, 65536)), dim3(kThreads), 0, s, A, b.s, b.r0,
                       b.rows, b.len, R.keys_out);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_strain_ranks_dev(const long long *d_j, const float *d_dist, const long long *seg_off,
                                    size_t n_strains, size_t depth, const int32_t *ranks, size_t n_ranks,
                                    int reciprocal_only, int count_unique_distances, float epsilon, int32_t *d_prefix,
                                    long long *d_pos_i, long long *d_pos_j, long long *d_level, float *d_level_dist,
                                    size_t cap, size_t *n_out, void *stream) {
  const std::string who = "ppk_strain_ranks";
  if (!n_out) return ppk_fail(PPK_ERR_ARG, who + ": n_out is NULL");
  *n_out = 0;
  if (!d_j || !d_dist || !ranks || !d_prefix) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (depth == 0) return ppk_fail(PPK_ERR_ARG, who + ": depth must be at least 1");
  if (n_ranks == 0 || n_ranks > (size_t)kMaxRanks) return ppk_fail(PPK_ERR_ARG, who + ": n_ranks must be 1 .. 1023");
  for (size_t q = 0; q < n_ranks; ++q)
    if (ranks[q] < 1 || (q > 0 && ranks[q] <= ranks[q - 1]))
      return ppk_fail(PPK_ERR_ARG, who + ": ranks must be at least 1 and ascending");
  size_t m = 0;
  int rc = lin_check_segments(who, seg_off, n_strains, &m);
  if (rc != PPK_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);

  const std::vector<long long> out_off = lin_out_offsets(seg_off, n_strains, depth);
  size_t scan_tmp = 0;
  PPK_HIP(rocprim::inclusive_scan(nullptr, scan_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr, m,
                                  rocprim::plus<unsigned long long>(), s));
  RankArgs A{};
  unsigned long long *bad, *cnt, *offs;
  long long *d_seg, *d_off;
  int32_t *d_ranks;
  char *tmp;
  rc = ppk_scratch_carve(dev, SLOT_LINEAGE, [&](Carve &c) {
    c.take(bad, 1).take(d_seg, n_strains + 1).take(d_off, n_strains + 1).take(d_ranks, n_ranks).take(cnt, m);
    c.take(offs, m + 1).take(tmp, scan_tmp + 256);
  });
  if (rc != PPK_OK) return rc;
  A.j = d_j;
  A.d = d_dist;
  A.seg_off = d_seg;
  A.out_off = d_off;
  A.ranks = d_ranks;
  A.n_strains = (int)n_strains;
  A.n_ranks = (int)n_ranks;
  A.m = m;
  A.depth = depth;
  A.reciprocal = reciprocal_only ? 1 : 0;
  A.count_unique = count_unique_distances ? 1 : 0;
  A.epsilon = epsilon;
  A.prefix = d_prefix;

  ppk_prof_stage("prefix", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  PPK_HIP(hipMemsetAsync(offs, 0, 8, s));
  PPK_HIP(hipMemcpyAsync(d_seg, seg_off, (n_strains + 1) * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_off, out_off.data(), (n_strains + 1) * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_ranks, ranks, n_ranks * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(lin_prefix_kernel, dim3(grid_for(m, kThreads, ~0u)), dim3(kThreads), 0, s, A, bad);
  ppk_prof_stage("stream", s);
  const dim3 grid(grid_for(m, kThreads / 64, ~0u));
  hipLaunchKernelGGL((lin_stream_kernel<false>), grid, dim3(kThreads), 0, s, A, cnt, nullptr, nullptr, nullptr, nullptr,
                     nullptr);
  PPK_HIP(hipGetLastError());
  size_t bytes = scan_tmp;
  PPK_HIP(rocprim::inclusive_scan(tmp, bytes, cnt, offs + 1, m, rocprim::plus<unsigned long long>(), s));
  // the call's one synchronisation: the first bad row and the entries of the stream
  const unsigned long long *h = nullptr;
  rc = ppk_read_back(dev, s, {{bad, 8}, {offs + m, 8}}, &h);
  if (rc != PPK_OK) {
    ppk_prof_stage(nullptr, s);
    return rc;
  }
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    const size_t g = (size_t)h[0], t = strain_of(seg_off, n_strains, g);
    return ppk_fail(PPK_ERR_ARG, who + ": strain " + std::to_string(t) + ", member " +
                                     std::to_string(g - (size_t)seg_off[t]) + ": a column outside [0, " +
                                     std::to_string(seg_off[t + 1] - seg_off[t]) + ") or the row itself");
  }
  const size_t total = (size_t)h[1];
  *n_out = total;
  if (total > cap) {
    ppk_prof_stage(nullptr, s);
    return ppk_fail(PPK_ERR_CAPACITY, who + ": output too small: need " + std::to_string(total));
  }
  if (total > 0) {
    if (!d_pos_i || !d_pos_j || !d_level) {
      ppk_prof_stage(nullptr, s);
      return ppk_fail(PPK_ERR_ARG, who + ": NULL output");
    }
    hipLaunchKernelGGL((lin_stream_kernel<true>), grid, dim3(kThreads), 0, s, A, nullptr, offs, d_pos_i, d_pos_j, d_level,
                       d_level_dist);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

// ---- host arrays ------------------------------------------------------------------------------------------------
extern "C" int ppk_strain_knn(const float *dist, size_t n, int dist_col, const long long *members,
                              const long long *seg_off, size_t n_strains, size_t depth, int device_id,
                              long long *i_out, long long *j_out, float *d_out) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const std::string who = "ppk_strain_knn";
  if (!dist || !members || !i_out || !j_out || !d_out) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (n < 2 || n >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n must be 2 .. 2^31 - 2");
  size_t m = 0;
  const int rc0 = lin_check_segments(who, seg_off, n_strains, &m);
  if (rc0 != PPK_OK) return rc0;
  const size_t n_rows = n * (n - 1) / 2;
  const size_t nnz = (size_t)lin_out_offsets(seg_off, n_strains, depth ? depth : 1).back();
  float *d_mat, *d_od;
  long long *d_members, *d_oi, *d_oj;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_mat, n_rows * 2).take(d_members, m).take(d_oi, nnz).take(d_oj, nnz).take(d_od, nnz);
  }, [&]() -> int {
    int rc = ppk_check_arch(device_id);
    if (rc == PPK_OK) rc = ppk_upload(device_id, d_mat, dist, n_rows * 8, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(d_members, members, m * 8, hipMemcpyHostToDevice));
    rc = ppk_strain_knn_dev(d_mat, n, dist_col, d_members, seg_off, n_strains, depth, d_oi, d_oj, d_od, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(i_out, d_oi, nnz * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(j_out, d_oj, nnz * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(d_out, d_od, nnz * 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" int ppk_strain_extend(const long long *members, const long long *seg_off, const long long *queries,
                                 const long long *qry_off, size_t n_strains, const long long *nn_j, const float *nn_d,
                                 const float *qr, const float *qq, size_t n_ref, size_t n_qry, int dist_col,
                                 float floor, size_t depth, int device_id, long long *i_out, long long *j_out,
                                 float *d_out) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const std::string who = "ppk_strain_extend";
  if (!members || !nn_j || !nn_d || !i_out || !j_out || !d_out) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (n_ref < 2 || n_ref >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n_ref must be 2 .. 2^31 - 2");
  if (n_qry >= (size_t)0x7fffffff) return ppk_fail(PPK_ERR_ARG, who + ": n_qry must be below 2^31 - 1");
  size_t m = 0, mq = 0;
  int rc0 = lin_check_segments(who, seg_off, n_strains, &m);
  if (rc0 != PPK_OK) return rc0;
  std::vector<long long> ext_seg;
  if ((rc0 = ext_check_queries(who, seg_off, qry_off, n_strains, &mq, &ext_seg)) != PPK_OK) return rc0;
  if (mq && (!queries || !qr)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const size_t nn = (size_t)lin_out_offsets(seg_off, n_strains, depth ? depth : 1).back();
  const size_t nnz = (size_t)lin_out_offsets(ext_seg.data(), n_strains, depth ? depth : 1).back();
  const size_t qr_rows = mq ? n_qry * n_ref : 0, qq_rows = qq ? n_qry * (n_qry - 1) / 2 : 0;
  float *d_qr, *d_qq, *d_nd, *d_od;
  long long *d_members, *d_queries, *d_nj, *d_oi, *d_oj;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_qr, qr_rows * 2).take(d_qq, qq_rows * 2).take(d_members, m).take(d_queries, mq).take(d_nj, nn);
    c.take(d_nd, nn).take(d_oi, nnz).take(d_oj, nnz).take(d_od, nnz);
  }, [&]() -> int {
    int rc = ppk_check_arch(device_id);
    if (rc == PPK_OK && qr_rows) rc = ppk_upload(device_id, d_qr, qr, qr_rows * 8, nullptr);
    if (rc == PPK_OK && qq_rows) rc = ppk_upload(device_id, d_qq, qq, qq_rows * 8, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(d_members, members, m * 8, hipMemcpyHostToDevice));
    if (mq) PPK_HIP(hipMemcpy(d_queries, queries, mq * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_nj, nn_j, nn * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_nd, nn_d, nn * 4, hipMemcpyHostToDevice));
    rc = ppk_strain_extend_dev(d_members, seg_off, mq ? d_queries : nullptr, qry_off, n_strains, d_nj, d_nd,
                               qr_rows ? d_qr : nullptr, qq_rows ? d_qq : nullptr, n_ref, n_qry, dist_col, floor, depth,
                               d_oi, d_oj, d_od, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(i_out, d_oi, nnz * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(j_out, d_oj, nnz * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(d_out, d_od, nnz * 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" int ppk_strain_ranks(const long long *j, const float *dist, const long long *seg_off, size_t n_strains,
                                size_t depth, const int32_t *ranks, size_t n_ranks, int reciprocal_only,
                                int count_unique_distances, float epsilon, int device_id, int32_t *prefix,
                                long long *pos_i, long long *pos_j, long long *level, float *level_dist, size_t cap,
                                size_t *n_out) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const std::string who = "ppk_strain_ranks";
  if (!n_out) return ppk_fail(PPK_ERR_ARG, who + ": n_out is NULL");
  *n_out = 0;
  if (!j || !dist || !ranks || !prefix) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (depth == 0) return ppk_fail(PPK_ERR_ARG, who + ": depth must be at least 1");
  if (n_ranks == 0 || n_ranks > (size_t)kMaxRanks) return ppk_fail(PPK_ERR_ARG, who + ": n_ranks must be 1 .. 1023");
  size_t m = 0;
  const int rc0 = lin_check_segments(who, seg_off, n_strains, &m);
  if (rc0 != PPK_OK) return rc0;
  const size_t nnz = (size_t)lin_out_offsets(seg_off, n_strains, depth).back();
  const size_t room = cap < nnz ? cap : nnz;           // (the stream never holds more than the lists)
  long long *d_j, *d_pi, *d_pj, *d_lv;
  float *d_d, *d_ld;
  int32_t *d_prefix;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_j, nnz).take(d_d, nnz).take(d_prefix, n_ranks * m).take(d_pi, room).take(d_pj, room).take(d_lv, room);
    c.take(d_ld, room);
  }, [&]() -> int {
    int rc = ppk_check_arch(device_id);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(d_j, j, nnz * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_d, dist, nnz * 4, hipMemcpyHostToDevice));
    rc = ppk_strain_ranks_dev(d_j, d_d, seg_off, n_strains, depth, ranks, n_ranks, reciprocal_only,
                              count_unique_distances, epsilon, d_prefix, d_pi, d_pj, d_lv, d_ld, room, n_out, nullptr);
    if (rc == PPK_ERR_CAPACITY || rc == PPK_OK) PPK_HIP(hipMemcpy(prefix, d_prefix, n_ranks * m * 4, hipMemcpyDeviceToHost));
    if (rc != PPK_OK) return rc;
    const size_t total = *n_out;
    if (total) {
      if (!pos_i || !pos_j || !level) return ppk_fail(PPK_ERR_ARG, who + ": NULL output");
      PPK_HIP(hipMemcpy(pos_i, d_pi, total * 8, hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(pos_j, d_pj, total * 8, hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(level, d_lv, total * 8, hipMemcpyDeviceToHost));
      if (level_dist) PPK_HIP(hipMemcpy(level_dist, d_ld, total * 4, hipMemcpyDeviceToHost));
    }
    return PPK_OK;
  });
}

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
// of c's sorted row: the same long-form element, so the same distance, found by bisection on (key of the distance,
// column).  An unordered pair goes out once: where both directions are kept, from the lower row, at the earlier of the
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
        int lo = 0, hi = last[g2];                    // the first place of c's kept part not before (key, r)
        while (lo < hi) {
          const int mid = (lo + hi) / 2;
          const unsigned k2 = ord_of(A.d[base2 + mid]);
          const long long j2 = A.j[base2 + mid];
          if (k2 < key || (k2 == key && j2 < r)) lo = mid + 1;
          else hi = mid;
        }
        const bool both = lo < last[g2] && A.j[base2 + lo] == r && ord_of(A.d[base2 + lo]) == key;
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

// the offsets of the sorted lists: out_off[s] = the entries of the strains before s
std::vector<long long> lin_out_offsets(const long long *seg_off, size_t n_strains, size_t depth) {
  std::vector<long long> out(n_strains + 1, 0);
  for (size_t s = 0; s < n_strains; ++s) {
    const size_t n_s = (size_t)(seg_off[s + 1] - seg_off[s]);
    out[s + 1] = out[s] + (long long)(n_s * (depth < n_s - 1 ? depth : n_s - 1));
  }
  return out;
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

  // routing, on the host: the wave and LDS routes' strains with the rows before each, the long route's bands
  long long lds_max = ppk_config().lineage_lds_keys.load();
  if (lds_max <= 0 || lds_max > kLdsKeys) lds_max = kLdsKeys;
  const long long cap_mb = ppk_config().lineage_scratch_mb.load();
  const size_t room = ((size_t)(cap_mb > 0 ? cap_mb : 0) << 20) / 5 * 4;      // (a slot is allocated with a quarter to spare)
  const std::vector<long long> out_off = lin_out_offsets(seg_off, n_strains, depth);
  std::vector<int32_t> wave_s, lds_s;
  std::vector<long long> wave_rows(1, 0), lds_rows(1, 0);
  struct Band {
    int s;
    long long r0;
    size_t rows, len;
  };
  std::vector<Band> bands;
  size_t most_keys = 0, tmp_bytes = 0;
  for (size_t t = 0; t < n_strains; ++t) {
    const size_t n_s = (size_t)(seg_off[t + 1] - seg_off[t]), len = n_s - 1;
    if (len <= (size_t)kWaveKeys) {
      wave_s.push_back((int32_t)t);
      wave_rows.push_back(wave_rows.back() + (long long)n_s);
    } else if (len <= (size_t)lds_max) {
      lds_s.push_back((int32_t)t);
      lds_rows.push_back(lds_rows.back() + (long long)n_s);
    } else {
      if (len >= kSortItems) return ppk_fail(PPK_ERR_ARG, who + ": a strain of 2^31 members or more");
      size_t rows = room / (len * 2 * sizeof(uint64_t));      // both key buffers of a band under the cap; at least a row
      if (rows > kSortItems / len) rows = kSortItems / len;
      if (rows < 1) rows = 1;
      if (rows > n_s) rows = n_s;
      for (size_t r0 = 0; r0 < n_s; r0 += rows) {
        const size_t take = r0 + rows < n_s ? rows : n_s - r0;
        bands.push_back(Band{(int)t, (long long)r0, take, len});
      }
      if (rows * len > most_keys) most_keys = rows * len;
      size_t bytes = 0;
      const auto begin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0), TimesLen{(unsigned)len});
      PPK_HIP(rocprim::segmented_radix_sort_keys(nullptr, bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                 (unsigned)(rows * len), (unsigned)rows, begin, begin + 1, 0u, 64u, s));
      if (bytes > tmp_bytes) tmp_bytes = bytes;
    }
  }

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
  int32_t *owner, *d_wave_s, *d_lds_s;
  long long *d_seg, *d_off, *d_wave_rows, *d_lds_rows;
  uint64_t *keys_in, *keys_out;
  char *tmp;
  rc = ppk_scratch_carve(dev, SLOT_LINEAGE, [&](Carve &c) {
    c.take(bad, 2).take(owner, n).take(d_seg, n_strains + 1).take(d_off, n_strains + 1);
    c.take(d_wave_s, wave_s.size()).take(d_wave_rows, wave_rows.size()).take(d_lds_s, lds_s.size());
    c.take(d_lds_rows, lds_rows.size()).take(keys_in, most_keys).take(keys_out, most_keys).take(tmp, tmp_bytes + 256);
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
  if (!wave_s.empty()) {
    PPK_HIP(hipMemcpyAsync(d_wave_s, wave_s.data(), wave_s.size() * 4, hipMemcpyHostToDevice, s));
    PPK_HIP(hipMemcpyAsync(d_wave_rows, wave_rows.data(), wave_rows.size() * 8, hipMemcpyHostToDevice, s));
  }
  if (!lds_s.empty()) {
    PPK_HIP(hipMemcpyAsync(d_lds_s, lds_s.data(), lds_s.size() * 4, hipMemcpyHostToDevice, s));
    PPK_HIP(hipMemcpyAsync(d_lds_rows, lds_rows.data(), lds_rows.size() * 8, hipMemcpyHostToDevice, s));
  }
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

  if (!wave_s.empty()) {
    ppk_prof_stage("wave", s);
    const long long total = wave_rows.back();
    hipLaunchKernelGGL(lin_wave_kernel, dim3(grid_for((size_t)total, kThreads / 64, ~0u)), dim3(kThreads), 0, s, A,
                       d_wave_s, d_wave_rows, (int)wave_s.size(), total);
  }
  if (!lds_s.empty()) {
    ppk_prof_stage("lds", s);
    hipLaunchKernelGGL(lin_lds_kernel, dim3((unsigned)lds_rows.back()), dim3(kThreads), 0, s, A, d_lds_s, d_lds_rows,
                       (int)lds_s.size());
  }
  PPK_HIP(hipGetLastError());
  if (!bands.empty()) ppk_prof_stage("long", s);
  for (const Band &b : bands) {
    const size_t items = b.rows * b.len;
    hipLaunchKernelGGL(lin_fill_kernel, dim3(grid_for(items, kThreads * 4, 65536)), dim3(kThreads), 0, s, A, b.s, b.r0,
                       items, keys_in);
    size_t bytes = tmp_bytes;
    const auto begin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0), TimesLen{(unsigned)b.len});
    PPK_HIP(rocprim::segmented_radix_sort_keys(tmp, bytes, (const uint64_t *)keys_in, keys_out, (unsigned)items,
                                               (unsigned)b.rows, begin, begin + 1, 0u, 64u, s));
    hipLaunchKernelGGL(lin_emit_kernel, dim3(grid_for(items, kThreads * 4, 65536)), dim3(kThreads), 0, s, A, b.s, b.r0,
                       b.rows, keys_out);
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

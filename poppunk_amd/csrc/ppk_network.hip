// Network scores of refine's boundary sweep on the device.
//
//  - ppk_network_sweep_dev : the integer counts behind PopPUNK/network.py:1204-1307 (networkSummary, graph-tool
//    branch, no betweenness) for every graph G_t of a growing sequence, as refine.growNetwork (PopPUNK/refine.py:
//    375-474) builds it: G_t holds every edge whose offset index is <= t, over vertices 0 .. n-1.  Per t:
//    {|E(G_t)|, connected components, triangles T, connected triples W = sum_v C(d_v, 2)}.
//    Stages (ppk_prof_stages names):
//      validate    one pass checks every id and offset index and counts the edges per offset (LDS histogram);
//                  the call's ONE synchronisation reads those counts and the first bad edge
//      csr         the edges bucketed by offset (rocPRIM scan of the counts, workgroup-reserved ranges), and both
//                  directions of every edge radix-sorted (rocPRIM) by (row, neighbour > row, offset): each row is
//                  its lower neighbours then its higher ones, each part in offset order
//      components  lock-free union-find, one launch per non-empty offset batch in order: a root links under the
//                  smaller root by CAS, so each success removes one component (components[t] = n - links so far);
//                  optional labels after batch labels_at (root = the smallest vertex of its set, dense-ranked)
//      wedges      a row entry at position k of the row's offset order closes k wedges, all at its own offset
//                  (the larger of the two edges'); per-workgroup LDS histogram
//      triangles   edges oriented low -> high id; one workgroup per source u puts N+(u)'s offset indices in an LDS
//                  table indexed by w and probes it for every w in N+(v), v in N+(u): each triangle is found once,
//                  at u = its smallest vertex, and counted at the largest offset of its three edges
//    then one small kernel prefix-sums the per-offset increments into the [n_off][4] result.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <string>
#include <vector>

#include "ppk_internal.h"

namespace {

constexpr int kMaxOff = 1023;          // offsets per call, as the sweeps (ppk_iterate.hip)
constexpr int kOffBits = 10;           // an offset index in a sort key / the LDS table (value + 1 in 16 bits)
constexpr int kThreads = 256;
constexpr int kScatterItems = 16;      // edges per thread of one scatter chunk
// LDS table of the triangle stage: 16-bit entries, one per vertex id of the window.  144 KiB + the 8 KiB histogram
// stay under the 160 KiB a workgroup may declare (MI355X_MICROARCH.md, LDS); graphs of more vertices go in windows.
constexpr size_t kTableMax = 73728;
constexpr size_t kTableSmall = 24576;  // ... when the launch cannot be given more than 64 KiB of dynamic LDS

__device__ __forceinline__ int ld_relaxed(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Per-lane run of one histogram bin: consecutive adds to the same bin (the common case: rows are in offset order)
// cost one LDS atomic per run instead of one per add.
struct BinRun {
  int bin = -1;
  unsigned long long c = 0;
  __device__ __forceinline__ void add(unsigned long long *hist, int b, unsigned long long v) {
    if (b != bin) {
      if (c) atomicAdd(&hist[bin], c);
      bin = b;
      c = 0;
    }
    c += v;
  }
  __device__ __forceinline__ void flush(unsigned long long *hist) {
    if (c) atomicAdd(&hist[bin], c);
    c = 0;
  }
};

__device__ __forceinline__ void hist_clear(unsigned long long *hist, int n_off) {
  for (int b = threadIdx.x; b < n_off; b += blockDim.x) hist[b] = 0;
}
__device__ __forceinline__ void hist_flush(const unsigned long long *hist, int n_off, unsigned long long *out) {
  for (int b = threadIdx.x; b < n_off; b += blockDim.x)
    if (hist[b]) atomicAdd(&out[b], hist[b]);
}

// ---- validate: ids, self-loops, offsets; edges per offset ------------------------------------------------------
__global__ void __launch_bounds__(kThreads) net_validate_kernel(const long long *ei, const long long *ej, size_t stride,
                                                                const long long *eo, size_t m, long long n, int n_off,
                                                                unsigned *cnt, unsigned long long *bad) {
  __shared__ unsigned hist[kMaxOff + 1];
  for (int b = threadIdx.x; b < n_off; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const long long i = ei[k * stride], j = ej[k * stride], o = eo ? eo[k] : 0;
    const bool ok = i >= 0 && i < n && j >= 0 && j < n && i != j && o >= 0 && o < n_off;
    if (ok) atomicAdd(&hist[o], 1u);
    else atomicMin(bad, (unsigned long long)k);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_off; b += blockDim.x)
    if (hist[b]) atomicAdd(&cnt[b], hist[b]);
}

// ---- csr: bucket by offset, both directions of every edge as (key, neighbour) ---------------------------------
// Each workgroup takes a chunk of kThreads * kScatterItems edges, ranks them per offset in LDS, reserves its range of
// every bucket with one atomic per non-empty bin, and writes.  Positions inside a bucket are in no particular order
// (the union-find does not care).  key = row << 11 | (neighbour > row) << 10 | offset.
__global__ void __launch_bounds__(kThreads) net_scatter_kernel(const long long *ei, const long long *ej, size_t stride,
                                                               const long long *eo, size_t m, int n_off,
                                                               unsigned *cursor, int *bu, int *bv,
                                                               unsigned long long *keys, int *vals) {
  __shared__ unsigned lcnt[kMaxOff + 1];
  __shared__ unsigned base[kMaxOff + 1];
  const size_t chunk = (size_t)kThreads * kScatterItems;
  for (size_t c0 = (size_t)blockIdx.x * chunk; c0 < m; c0 += (size_t)gridDim.x * chunk) {
    for (int b = threadIdx.x; b < n_off; b += blockDim.x) lcnt[b] = 0;
    __syncthreads();
    unsigned rank[kScatterItems];
#pragma unroll
    for (int q = 0; q < kScatterItems; ++q) {
      const size_t k = c0 + (size_t)q * kThreads + threadIdx.x;
      rank[q] = 0;
      if (k < m) {
        const int o = eo ? (int)eo[k] : 0;
        rank[q] = atomicAdd(&lcnt[o], 1u);
      }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_off; b += blockDim.x)
      if (lcnt[b]) base[b] = atomicAdd(&cursor[b], lcnt[b]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kScatterItems; ++q) {
      const size_t k = c0 + (size_t)q * kThreads + threadIdx.x;
      if (k < m) {
        const int i = (int)ei[k * stride], j = (int)ej[k * stride];
        const int o = eo ? (int)eo[k] : 0;
        const unsigned pos = base[o] + rank[q];
        bu[pos] = i;
        bv[pos] = j;
        keys[2 * k] = ((unsigned long long)i << 11) | ((unsigned long long)(j > i) << 10) | (unsigned)o;
        vals[2 * k] = j;
        keys[2 * k + 1] = ((unsigned long long)j << 11) | ((unsigned long long)(i > j) << 10) | (unsigned)o;
        vals[2 * k + 1] = i;
      }
    }
    __syncthreads();
  }
}

// Segment starts of the sorted entries: segment 2r = row r's lower neighbours, 2r + 1 its higher ones; start2 has
// 2n + 1 entries (start2[2n] = 2m).  Each entry fills the starts of the segments between its predecessor's and its
// own; the last one those after it.  Also the entries' offsets as 16-bit values.
__global__ void __launch_bounds__(kThreads) net_segments_kernel(const unsigned long long *keys, size_t e, size_t n_seg,
                                                                unsigned *start2, uint16_t *off16) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[p];
    const size_t sg = key >> kOffBits;
    off16[p] = (uint16_t)(key & ((1u << kOffBits) - 1));
    const size_t first = p ? (keys[p - 1] >> kOffBits) + 1 : 0;
    for (size_t x = first; x <= sg; ++x) start2[x] = (unsigned)p;
    if (p == e - 1)
      for (size_t x = sg + 1; x <= n_seg; ++x) start2[x] = (unsigned)e;
  }
}

// ---- components ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) net_parent_init_kernel(int *parent, size_t n) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    parent[v] = (int)v;
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

// one offset batch: link the two roots of every edge; links[t] += the successful links
__global__ void __launch_bounds__(kThreads) net_union_kernel(const int *bu, const int *bv, unsigned len, int *parent,
                                                             unsigned *links_t) {
  unsigned mine = 0;
  for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < len; k += gridDim.x * blockDim.x) {
    int a = bu[k], b = bv[k];
    while (true) {
      a = uf_find(parent, a);
      b = uf_find(parent, b);
      if (a == b) break;
      const int hi = a > b ? a : b, lo = a > b ? b : a;
      if (atomicCAS(parent + hi, hi, lo) == hi) {
        ++mine;
        break;
      }
    }
  }
  __shared__ unsigned acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  if (mine) atomicAdd(&acc, mine);
  __syncthreads();
  const unsigned tot = acc;
  if (threadIdx.x == 0 && tot) atomicAdd(links_t, tot);
}

// labels: is_root[v] = (v is a root), then (after the scan) label[v] = rank of v's root
__global__ void __launch_bounds__(kThreads) net_roots_kernel(const int *parent, size_t n, int *is_root) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    is_root[v] = parent[v] == (int)v;
}
__global__ void __launch_bounds__(kThreads) net_labels_kernel(const int *parent, size_t n, const int *rank,
                                                              int32_t *labels) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    int x = (int)v;
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    labels[v] = rank[x];
  }
}

// ---- wedges ------------------------------------------------------------------------------------------------------
// pairs of one row's entries, each counted once at the entry with the larger offset (ties: the later position).
// An entry of the lower part at index k: k earlier lower entries, plus the higher entries of offset <= its own; one
// of the higher part: k earlier higher entries, plus the lower entries of offset < its own.
__device__ __forceinline__ unsigned count_below(const uint16_t *off, unsigned lo, unsigned hi, unsigned t, bool incl) {
  while (lo < hi) {
    const unsigned mid = lo + (hi - lo) / 2;
    const unsigned v = off[mid];
    if (v < t || (incl && v == t)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__global__ void __launch_bounds__(kThreads) net_wedges_kernel(const unsigned long long *keys, const uint16_t *off16,
                                                              const unsigned *start2, size_t e, int n_off,
                                                              unsigned long long *wedges) {
  __shared__ unsigned long long hist[kMaxOff + 1];
  hist_clear(hist, n_off);
  __syncthreads();
  BinRun run;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[p];
    const size_t r = key >> (kOffBits + 1);
    const bool high = (key >> kOffBits) & 1;
    const unsigned t = (unsigned)(key & ((1u << kOffBits) - 1));
    const unsigned a0 = start2[2 * r], a1 = start2[2 * r + 1], a2 = start2[2 * r + 2];
    unsigned c;
    if (!high) c = ((unsigned)p - a0) + (count_below(off16, a1, a2, t, true) - a1);
    else c = ((unsigned)p - a1) + (count_below(off16, a0, a1, t, false) - a0);
    if (c) run.add(hist, (int)t, c);
  }
  run.flush(hist);
  __syncthreads();
  hist_flush(hist, n_off, wedges);
}

// ---- triangles ---------------------------------------------------------------------------------------------------
// One workgroup per source vertex u (grid-stride).  N+(u) = row u's higher part.  For a window [w0, w0 + W) of ids,
// table[w - w0] = offset(u, w) + 1 for w in N+(u); every wave takes a v of N+(u) and its lanes walk N+(v): a hit
// at w is the triangle (u, v, w), counted at max(offset(u,v), offset(v,w), offset(u,w)).  Only the entries that were
// set are cleared again.
__global__ void __launch_bounds__(kThreads) net_triangles_kernel(const int *nbr, const uint16_t *off16,
                                                                 const unsigned *start2, size_t n, int n_off,
                                                                 unsigned table_len, unsigned long long *tri) {
  extern __shared__ uint16_t table[];
  __shared__ unsigned long long hist[kMaxOff + 1];
  __shared__ int wmin, wmax;
  hist_clear(hist, n_off);
  for (unsigned k = threadIdx.x; k < table_len; k += blockDim.x) table[k] = 0;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  BinRun run;
  for (size_t u = blockIdx.x; u < n; u += gridDim.x) {
    const unsigned h0 = start2[2 * u + 1], h1 = start2[2 * u + 2];
    if (h1 - h0 < 2) continue;                       // (uniform) u is the smallest vertex of no triangle
    if (threadIdx.x == 0) {
      wmin = 0x7fffffff;
      wmax = -1;
    }
    __syncthreads();
    for (unsigned k = h0 + threadIdx.x; k < h1; k += blockDim.x) {
      atomicMin(&wmin, nbr[k]);
      atomicMax(&wmax, nbr[k]);
    }
    __syncthreads();
    const long long lo_id = wmin, hi_id = wmax;
    for (long long w0 = lo_id; w0 <= hi_id; w0 += table_len) {
      for (unsigned k = h0 + threadIdx.x; k < h1; k += blockDim.x) {
        const unsigned long long d = (unsigned long long)((long long)nbr[k] - w0);
        if (d < table_len) table[d] = (uint16_t)(off16[k] + 1);
      }
      __syncthreads();
      for (unsigned vi = h0 + wave; vi < h1; vi += n_waves) {
        const int v = nbr[vi];
        if ((long long)v >= hi_id) continue;         // N+(v) lies above every w of N+(u)
        const unsigned ouv = off16[vi];
        const unsigned q0 = start2[2 * (size_t)v + 1], q1 = start2[2 * (size_t)v + 2];
        for (unsigned q = q0 + lane; q < q1; q += 64) {
          const unsigned long long d = (unsigned long long)((long long)nbr[q] - w0);
          if (d < table_len) {
            const unsigned tw = table[d];
            if (tw) {
              unsigned b = off16[q];
              b = b > ouv ? b : ouv;
              b = b > tw - 1 ? b : tw - 1;
              run.add(hist, (int)b, 1);
            }
          }
        }
      }
      __syncthreads();
      for (unsigned k = h0 + threadIdx.x; k < h1; k += blockDim.x) {
        const unsigned long long d = (unsigned long long)((long long)nbr[k] - w0);
        if (d < table_len) table[d] = 0;
      }
      __syncthreads();
    }
  }
  run.flush(hist);
  __syncthreads();
  hist_flush(hist, n_off, tri);
}

// ---- result: prefix sums of the per-offset increments ------------------------------------------------------------
__global__ void net_stats_kernel(const unsigned *cnt, const unsigned *links, const unsigned long long *tri,
                                 const unsigned long long *wedges, long long n, int n_off, long long *stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long e = 0, l = 0, t = 0, w = 0;
  for (int o = 0; o < n_off; ++o) {
    e += cnt[o];
    l += links[o];
    t += (long long)tri[o];
    w += (long long)wedges[o];
    stats[4 * o + 0] = e;
    stats[4 * o + 1] = n - l;
    stats[4 * o + 2] = t;
    stats[4 * o + 3] = w;
  }
}

unsigned grid_for(size_t items, size_t per_block, unsigned cap) {
  size_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g < cap ? g : cap);
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// one pinned block per device for the call's one read-back: the first bad edge and the per-offset counts
unsigned long long *pinned_counts(int dev) {
  static unsigned long long *blocks[64] = {};
  if (dev < 0 || dev >= 64) return nullptr;
  if (!blocks[dev] && hipHostMalloc(reinterpret_cast<void **>(&blocks[dev]), 8 + (kMaxOff + 1) * 4 + 256,
                                    hipHostMallocDefault) != hipSuccess)
    blocks[dev] = nullptr;
  return blocks[dev];
}

// the LDS table of the triangle stage: the whole id range where it fits, else windows (option "net_window" forces a
// smaller one: tests of the windowed path)
unsigned table_entries(size_t n, bool big_lds) {
  size_t w = big_lds ? kTableMax : kTableSmall;
  const long long forced = ppk_config().net_window.load();
  if (forced > 0 && (size_t)forced < w) w = (size_t)forced;
  if (n < w) w = n;
  if (w < 1) w = 1;
  return (unsigned)((w + 1) & ~(size_t)1);
}

int bad_edge_message(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off, size_t k,
                     size_t n, size_t n_off) {
  long long i = 0, j = 0, o = 0;
  if (hipMemcpy(&i, d_i + k * stride, 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&j, d_j + k * stride, 8, hipMemcpyDeviceToHost) != hipSuccess ||
      (d_off && hipMemcpy(&o, d_off + k, 8, hipMemcpyDeviceToHost) != hipSuccess))
    return ppk_fail(PPK_ERR_HIP, "ppk_network_sweep: cannot read back the bad edge");
  std::string why;
  if (i < 0 || (size_t)i >= n || j < 0 || (size_t)j >= n) why = "vertex id out of range [0, " + std::to_string(n) + ")";
  else if (i == j) why = "self-loop";
  else why = "offset index out of range [0, " + std::to_string(n_off) + ")";
  return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: edge " + std::to_string(k) + " (i=" + std::to_string(i) +
                                   ", j=" + std::to_string(j) + ", offset " + std::to_string(o) + "): " + why);
}

}  // namespace

extern "C" int ppk_network_sweep_dev(const long long *d_i, const long long *d_j, size_t stride,
                                     const long long *d_off, size_t n_edges, size_t n_vertices, size_t n_off,
                                     long long labels_at, long long *d_stats, int32_t *d_labels, void *stream) {
  if (n_off == 0 || n_off > (size_t)kMaxOff) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: n_off must be 1 .. 1023");
  if (!d_off && n_off != 1 && n_edges)
    return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: no offset array needs n_off == 1");
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: n_vertices must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: n_edges must be < 2^31");
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: stride must be 1 or 2");
  if (labels_at < -1 || labels_at >= (long long)n_off)
    return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: labels_at must be -1 or an offset index");
  if (!d_stats || (labels_at >= 0 && !d_labels && n_vertices) || (n_edges && (!d_i || !d_j)))
    return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n_edges, n = n_vertices, e = 2 * m, no = n_off;

  // scratch layout (one slot): counters | parent | segment starts | buckets | keys x2 | values x2 | offsets | temp
  unsigned end_bit = kOffBits + 1;       // key bits: row id above the direction bit and the offset
  while (end_bit < 64 && ((size_t)1 << (end_bit - kOffBits - 1)) < n) ++end_bit;
  size_t sort_tmp = 0, scan_tmp = 0, scan_tmp2 = 0;
  if (e)
    PPK_HIP(rocprim::radix_sort_pairs(nullptr, sort_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                      (int *)nullptr, (int *)nullptr, e, 0u, end_bit, s));
  PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, (unsigned *)nullptr, (unsigned *)nullptr, 0u, no,
                                  rocprim::plus<unsigned>(), s));
  if (n) PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp2, (int *)nullptr, (int *)nullptr, 0, n, rocprim::plus<int>(), s));
  const size_t tmp = sort_tmp > scan_tmp ? (sort_tmp > scan_tmp2 ? sort_tmp : scan_tmp2) : (scan_tmp > scan_tmp2 ? scan_tmp : scan_tmp2);
  const size_t cnt_b = align256(1024 * 4), big_b = align256(1024 * 8);
  size_t at = 0;
  const size_t o_bad = at; at += 256;
  const size_t o_cnt = at; at += cnt_b;
  const size_t o_cur = at; at += cnt_b;
  const size_t o_links = at; at += cnt_b;
  const size_t o_tri = at; at += big_b;
  const size_t o_wed = at; at += big_b;
  const size_t zero_end = at;
  const size_t o_parent = at; at += align256(n * 4);
  const size_t o_root = at; at += align256(n * 4);
  const size_t o_rank = at; at += align256(n * 4);
  const size_t o_start = at; at += align256((2 * n + 1) * 4);
  const size_t o_bu = at; at += align256(m * 4);
  const size_t o_bv = at; at += align256(m * 4);
  const size_t o_ka = at; at += align256(e * 8);
  const size_t o_kb = at; at += align256(e * 8);
  const size_t o_va = at; at += align256(e * 4);
  const size_t o_vb = at; at += align256(e * 4);
  const size_t o_off = at; at += align256(e * 2);
  const size_t o_tmp = at; at += align256(tmp + 16);
  void *base = nullptr;
  int rc = ppk_scratch_get(dev, SLOT_NET, at, &base);
  if (rc != PPK_OK) return rc;
  char *B = static_cast<char *>(base);
  unsigned long long *bad = reinterpret_cast<unsigned long long *>(B + o_bad);
  unsigned *cnt = reinterpret_cast<unsigned *>(B + o_cnt), *cursor = reinterpret_cast<unsigned *>(B + o_cur);
  unsigned *links = reinterpret_cast<unsigned *>(B + o_links);
  unsigned long long *tri = reinterpret_cast<unsigned long long *>(B + o_tri);
  unsigned long long *wed = reinterpret_cast<unsigned long long *>(B + o_wed);
  int *parent = reinterpret_cast<int *>(B + o_parent), *is_root = reinterpret_cast<int *>(B + o_root);
  int *rank = reinterpret_cast<int *>(B + o_rank);
  unsigned *start2 = reinterpret_cast<unsigned *>(B + o_start);
  int *bu = reinterpret_cast<int *>(B + o_bu), *bv = reinterpret_cast<int *>(B + o_bv);
  unsigned long long *ka = reinterpret_cast<unsigned long long *>(B + o_ka), *kb = reinterpret_cast<unsigned long long *>(B + o_kb);
  int *va = reinterpret_cast<int *>(B + o_va), *vb = reinterpret_cast<int *>(B + o_vb);
  uint16_t *off16 = reinterpret_cast<uint16_t *>(B + o_off);
  void *d_tmp = B + o_tmp;
  unsigned long long *h = pinned_counts(dev);
  if (!h) return ppk_fail(PPK_ERR_HIP, "hipHostMalloc failed");

  // -- validate: the one synchronisation
  ppk_prof_stage("validate", s);
  PPK_HIP(hipMemsetAsync(B + o_cnt, 0, zero_end - o_cnt, s));
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  const unsigned cap_grid = 2048;
  if (m)
    hipLaunchKernelGGL(net_validate_kernel, dim3(grid_for(m, kThreads * 8, cap_grid)), dim3(kThreads), 0, s, d_i, d_j,
                       stride, d_off, m, (long long)n, (int)no, cnt, bad);
  PPK_HIP(hipGetLastError());
  PPK_HIP(hipMemcpyAsync(h, bad, 8, hipMemcpyDeviceToHost, s));
  PPK_HIP(hipMemcpyAsync(h + 1, cnt, no * 4, hipMemcpyDeviceToHost, s));
  PPK_HIP(hipStreamSynchronize(s));
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return bad_edge_message(d_i, d_j, stride, d_off, (size_t)h[0], n, no);
  }
  std::vector<unsigned> counts(no), starts(no);
  memcpy(counts.data(), h + 1, no * 4);
  for (size_t o = 0, acc = 0; o < no; ++o) {
    starts[o] = (unsigned)acc;
    acc += counts[o];
  }

  // -- csr
  ppk_prof_stage("csr", s);
  const int *nbr = vb;
  if (m) {
    size_t tb = tmp;
    PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, cnt, cursor, 0u, no, rocprim::plus<unsigned>(), s));
    hipLaunchKernelGGL(net_scatter_kernel, dim3(grid_for(m, (size_t)kThreads * kScatterItems, 4096)), dim3(kThreads), 0,
                       s, d_i, d_j, stride, d_off, m, (int)no, cursor, bu, bv, ka, va);
    PPK_HIP(hipGetLastError());
    tb = tmp;
    PPK_HIP(rocprim::radix_sort_pairs(d_tmp, tb, ka, kb, va, vb, e, 0u, end_bit, s));
    hipLaunchKernelGGL(net_segments_kernel, dim3(grid_for(e, kThreads, 8192)), dim3(kThreads), 0, s, kb, e, 2 * n,
                       start2, off16);
    PPK_HIP(hipGetLastError());
  }

  // -- components (+ labels after batch labels_at)
  ppk_prof_stage("components", s);
  hipLaunchKernelGGL(net_parent_init_kernel, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, s, parent, n);
  for (size_t o = 0; o < no; ++o) {
    if (counts[o])
      hipLaunchKernelGGL(net_union_kernel, dim3(grid_for(counts[o], kThreads * 4, 2048)), dim3(kThreads), 0, s,
                         bu + starts[o], bv + starts[o], counts[o], parent, links + o);
    if ((long long)o == labels_at && n) {
      hipLaunchKernelGGL(net_roots_kernel, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, s, parent, n, is_root);
      size_t tb = tmp;
      PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, is_root, rank, 0, n, rocprim::plus<int>(), s));
      hipLaunchKernelGGL(net_labels_kernel, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, s, parent, n, rank,
                         d_labels);
    }
  }
  PPK_HIP(hipGetLastError());

  if (m) {
    // -- wedges
    ppk_prof_stage("wedges", s);
    hipLaunchKernelGGL(net_wedges_kernel, dim3(grid_for(e, kThreads * 8, 2048)), dim3(kThreads), 0, s, kb, off16, start2,
                       e, (int)no, wed);
    PPK_HIP(hipGetLastError());
    // -- triangles
    ppk_prof_stage("triangles", s);
    static bool big_lds[64] = {}, asked[64] = {};
    if (!asked[dev & 63]) {
      asked[dev & 63] = true;
      big_lds[dev & 63] = hipFuncSetAttribute(reinterpret_cast<const void *>(net_triangles_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)(kTableMax * sizeof(uint16_t))) == hipSuccess;
      (void)hipGetLastError();
    }
    const unsigned tl = table_entries(n, big_lds[dev & 63]);
    hipLaunchKernelGGL(net_triangles_kernel, dim3((unsigned)(n < (1u << 20) ? n : (1u << 20))), dim3(kThreads),
                       tl * sizeof(uint16_t), s, nbr, off16, start2, n, (int)no, tl, tri);
    PPK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(net_stats_kernel, dim3(1), dim3(64), 0, s, cnt, links, tri, wed, (long long)n, (int)no, d_stats);
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_network_sweep(const long long *i, const long long *j, const long long *off, size_t n_edges,
                                 size_t n_vertices, size_t n_off, int device_id, long long labels_at, long long *stats,
                                 int32_t *labels) {
  if (!stats || (n_edges && (!i || !j)) || (labels_at >= 0 && !labels && n_vertices))
    return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: NULL array");
  if (n_off == 0 || n_off > (size_t)kMaxOff) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: n_off must be 1 .. 1023");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: n_edges must be < 2^31");
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: n_vertices must be < 2^31");
  DeviceGuard guard(device_id);
  if (!guard.ok) return ppk_fail(PPK_ERR_HIP, "cannot select device " + std::to_string(device_id));
  PpkCall call(device_id, nullptr);
  const size_t eb = align256(n_edges * 8), sb = align256(n_off * 32), lb = align256(n_vertices * 4);
  void *p = nullptr;
  int rc = ppk_scratch_get(device_id, SLOT_HOST_IN, 3 * eb + sb + lb + 256, &p);
  if (rc != PPK_OK) return rc;
  char *B = static_cast<char *>(p);
  long long *d_i = reinterpret_cast<long long *>(B), *d_j = reinterpret_cast<long long *>(B + eb);
  long long *d_o = off ? reinterpret_cast<long long *>(B + 2 * eb) : nullptr;
  long long *d_stats = reinterpret_cast<long long *>(B + 3 * eb);
  int32_t *d_labels = reinterpret_cast<int32_t *>(B + 3 * eb + sb);
  if (n_edges) {
    PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
    if (off) PPK_HIP(hipMemcpy(d_o, off, n_edges * 8, hipMemcpyHostToDevice));
  }
  rc = ppk_network_sweep_dev(d_i, d_j, 1, d_o, n_edges, n_vertices, n_off, labels_at, d_stats,
                             labels_at >= 0 ? d_labels : nullptr, nullptr);
  if (rc != PPK_OK) return rc;
  PPK_HIP(hipMemcpy(stats, d_stats, n_off * 32, hipMemcpyDeviceToHost));
  if (labels_at >= 0 && n_vertices) PPK_HIP(hipMemcpy(labels, d_labels, n_vertices * 4, hipMemcpyDeviceToHost));
  return PPK_OK;
}

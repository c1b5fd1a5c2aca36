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
//  - ppk_network_summary_dev : the same counts plus networkSummary's betweenness (network.py:1286-1307) for every
//    G_t: the stages above, then the betweenness stage below.
//  - ppk_network_summary_sampled_dev : the same with at most bt_sources sources per component (the reference's
//    betweenness_sample, network.py:1272-1287), and optionally every vertex's value in the whole graph
//    (vertex_betweenness, network.py:1310-1313): the same stages plus bt_sources.
//  - ppk_cluster_sweep_dev : printClusters' cluster numbers (PopPUNK/network.py:1538-1545) of every vertex in every
//    G_t, from the same validation, buckets and union launches (the section before the entry points).
//  - ppk_cluster_extend_dev : the same numbers for (a loaded network + new edges), the loaded network given by its
//    component labels alone: the cluster sweep with a seeded forest.
#include <climits>
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
// (the union-find does not care).  key = row << 11 | (neighbour > row) << 10 | offset; keys == nullptr: buckets only.
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
        if (!keys) continue;             // (the cluster sweep wants the buckets alone)
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

// one offset batch: link the two roots of every edge; links[t] += the successful links
__global__ void __launch_bounds__(kThreads) net_union_kernel(const int *bu, const int *bv, unsigned len, int *parent,
                                                             unsigned *links_t) {
  unsigned mine = 0;
  for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < len; k += gridDim.x * blockDim.x) {
    mine += uf_union(parent, bu[k], bv[k]);
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

// who: the entry point's name, which starts every message
int bad_edge_message(const std::string &who, const long long *d_i, const long long *d_j, size_t stride,
                     const long long *d_off, size_t k, size_t n, size_t n_off) {
  long long i = 0, j = 0, o = 0;
  if (!ppk_read_edge(d_i, d_j, stride, d_off, k, &i, &j, &o))
    return ppk_fail(PPK_ERR_HIP, who + ": cannot read back the bad edge");
  std::string why;
  if (i < 0 || (size_t)i >= n || j < 0 || (size_t)j >= n) why = "vertex id out of range [0, " + std::to_string(n) + ")";
  else if (i == j) why = "self-loop";
  else why = "offset index out of range [0, " + std::to_string(n_off) + ")";
  return ppk_fail(PPK_ERR_ARG, who + ": edge " + std::to_string(k) + " (i=" + std::to_string(i) +
                                   ", j=" + std::to_string(j) + ", offset " + std::to_string(o) + "): " + why);
}

// ---- betweenness ------------------------------------------------------------------------------
// After the counts, every distinct graph G_t (each offset that adds edges) is rebuilt from the same sorted adjacency
// and union-find, and its components of more than 3 vertices are scored with exact Brandes:
//   bt_relabel  roots and sizes from the union-find at t; those components ordered by (size desc, root), their
//               vertices given local ids ordered by (component, id); a local CSR of G_t with rows sorted by neighbour
//   bt_sources  (sampled calls only) [EXT] every component of more than k vertices keeps k sources: its vertices of
//               smallest (ppk_bt_sample_key(seed, global id), global id), found by one stable sort of (component, key)
//               over the local ids; a scan of the picked flags gives each such component its list of sources in
//               ascending local id.  Components of at most k vertices take no list: every vertex, the id range.
//   bt_plan     one workgroup splits every component into work items of a fixed number of sources, sized from the
//               component's work (sources x (adjacency + n_c)); the graph's ONE synchronisation reads the plan's header
//   bt_brandes  level-synchronous Brandes per source; a work item writes its partial sums, never adds into a shared one
//   bt_reduce   per vertex the partials in item order, normalised; per component the maximum; the two means
// Normalisation, S = the sum of the partials in item order, every factor converted to double first:
//   all n_c sources               S / ((n_c - 1) * (n_c - 2))
//   k < n_c sources               (S * n_c) / (k * ((n_c - 1) * (n_c - 2)))        (networkx 3.4.2's _rescale)
//   whole graph (d_values only)   the same with (n - 1) * (n - 2), n = n_vertices, in place of the component's product
constexpr int kBtItems = 1024;         // work items per graph the plan aims at (fixed: results do not depend on the GPU)
constexpr int kBtSmallCap = 256;       // the small-component path's LDS holds components up to this size
constexpr size_t kBtLdsBytes = 160 * 1024 - 64;   // dynamic LDS of the LDS-state path (static: a few scalars)
constexpr unsigned long long kNone = ~0ull;
enum { H_K, H_KBIG, H_KGLOB, H_ITEMS, H_ITEMS_GLOB, H_PARTIAL, H_SCORED, H_NC_GLOB, H_NC_LDS, H_WORK, H_ADJ,
       H_K4, H_LEN = 16 };

size_t bt_state_bytes(size_t nc) { return 36 * nc + 8; }

__global__ void __launch_bounds__(kThreads) bt_sizes_kernel(const int *parent, size_t n, int *root, int *size) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const int r = uf_find_ro(parent, (int)v);
    root[v] = r;
    atomicAdd(&size[r], 1);
  }
}

// one key per root of a component of at least min_nc vertices (4; 3 for whole-graph values): (n - size, root); every
// other vertex kNone
__global__ void __launch_bounds__(kThreads) bt_root_keys_kernel(const int *root, const int *size, size_t n, int min_nc,
                                                                unsigned long long *keys) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    keys[v] = (root[v] == (int)v && size[v] >= min_nc) ? ((unsigned long long)(n - size[v]) << 32 | v) : kNone;
}

// component c (sorted position): its rank at its root, its size (0 past the last component)
__global__ void __launch_bounds__(kThreads) bt_comps_kernel(const unsigned long long *sorted, const int *size,
                                                            size_t n, int *crank, int *csize) {
  for (size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x; c <= n; c += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = c < n ? sorted[c] : kNone;
    if (key == kNone) {
      csize[c] = 0;
    } else {
      const int r = (int)(key & 0xffffffffu);
      crank[r] = (int)c;
      csize[c] = size[r];
    }
  }
}

__global__ void __launch_bounds__(kThreads) bt_vertex_keys_kernel(const int *root, const int *size, const int *crank,
                                                                  size_t n, int min_nc, unsigned long long *keys,
                                                                  int *local) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const int r = root[v];
    keys[v] = size[r] >= min_nc ? ((unsigned long long)crank[r] << 32 | v) : kNone;
    local[v] = -1;
  }
}

__global__ void __launch_bounds__(kThreads) bt_local_kernel(const unsigned long long *sorted, size_t n, int *local,
                                                            int *order) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = sorted[p];
    if (key == kNone) continue;
    const int v = (int)(key & 0xffffffffu);
    local[v] = (int)p;
    order[p] = v;
  }
}

// the entries of G_t (offset <= t) whose row is a scored vertex, as (local row, local neighbour) keys, appended in
// any order (they are sorted next); the rest of the 2|E(G_t)| slots keep kNone
__global__ void __launch_bounds__(kThreads) bt_edges_kernel(const unsigned long long *keys, const int *nbr, size_t e,
                                                            unsigned t, const int *local, unsigned *fill,
                                                            unsigned long long *out) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = keys[p];
    const int lr = (key & ((1u << kOffBits) - 1)) <= t ? local[key >> (kOffBits + 1)] : -1;
    if (lr >= 0) out[atomicAdd(fill, 1u)] = (unsigned long long)lr << 32 | (unsigned)local[nbr[p]];
  }
}

// row starts of the local CSR (rstart has n_scored + 1 entries) and the neighbours as int
__global__ void __launch_bounds__(kThreads) bt_rows_kernel(const unsigned long long *sorted, size_t len,
                                                           const long long *hdr, unsigned *rstart, int *lnbr) {
  const size_t ns = (size_t)hdr[H_SCORED];
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < len; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = sorted[p];
    if (key == kNone) continue;
    const size_t row = key >> 32;
    lnbr[p] = (int)(key & 0xffffffffu);
    const size_t first = p ? (sorted[p - 1] >> 32) + 1 : 0;
    for (size_t x = first; x <= row; ++x) rstart[x] = (unsigned)p;
    if (p + 1 == len || sorted[p + 1] == kNone)
      for (size_t x = row + 1; x <= ns; ++x) rstart[x] = (unsigned)(p + 1);
  }
}

// component starts (exclusive scan of csize) and the scored-vertex count: a one-workgroup scan
__global__ void __launch_bounds__(kThreads) bt_starts_kernel(const int *csize, size_t n, int *cstart, long long *hdr) {
  __shared__ long long part[kThreads];
  const size_t per = (n + 1 + kThreads - 1) / kThreads, c0 = threadIdx.x * per;
  const size_t c1 = c0 + per < n + 1 ? c0 + per : n + 1;
  long long acc = 0;
  for (size_t c = c0; c < c1; ++c) acc += csize[c];
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    for (int k = 0; k < kThreads; ++k) {
      const long long x = part[k];
      part[k] = run;
      run += x;
    }
    hdr[H_SCORED] = run;
  }
  __syncthreads();
  acc = part[threadIdx.x];
  for (size_t c = c0; c < c1; ++c) {
    cstart[c] = (int)acc;
    acc += csize[c];
  }
  if (threadIdx.x == kThreads - 1) cstart[n + 1] = (int)acc;
}

// ---- bt_sources ----
// vkeys: the sorted (component, vertex) keys of bt_relabel, position = local id.  Sort key of local id p: (component,
// sample key of its vertex) in a component of more than k vertices, (component, 0) in the others, so that every
// component's segment stays at cstart[c]; the sort is stable and p ascends with the vertex id within a component, so
// equal keys stay in id order.
__global__ void __launch_bounds__(kThreads) bt_src_keys_kernel(const unsigned long long *vkeys, const int *csize,
                                                               const long long *hdr, size_t n, int k,
                                                               unsigned long long seed, unsigned long long *keys,
                                                               int *ids, int *flag) {
  const size_t ns = (size_t)hdr[H_SCORED];
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    unsigned long long key = kNone;
    if (p < ns) {
      const unsigned long long c = vkeys[p] >> 32, v = vkeys[p] & 0xffffffffu;
      key = c << 32 | (csize[c] > k ? ppk_bt_sample_key(seed, v) : 0u);
    }
    keys[p] = key;
    ids[p] = (int)p;
    flag[p] = 0;
  }
}
// position r of the sorted order has rank r - cstart[c] in its component: the first k of a sampled component are picked
__global__ void __launch_bounds__(kThreads) bt_src_pick_kernel(const unsigned long long *sorted, const int *ids,
                                                               const int *csize, const int *cstart,
                                                               const long long *hdr, int k, int *flag) {
  const size_t ns = (size_t)hdr[H_SCORED];
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < ns; r += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(sorted[r] >> 32);
    if (csize[c] > k && (long long)r - cstart[c] < k) flag[ids[r]] = 1;
  }
}
// pos = the exclusive scan of flag: the picked vertices of component c are src[sbase[c] .. + k), component-relative,
// in ascending local id
__global__ void __launch_bounds__(kThreads) bt_src_list_kernel(const unsigned long long *vkeys, const int *flag,
                                                               const int *pos, const int *cstart, const long long *hdr,
                                                               int *src, int *sbase) {
  const size_t ns = (size_t)hdr[H_SCORED];
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < ns; p += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(vkeys[p] >> 32), first = cstart[c];
    if ((int)p == first) sbase[c] = pos[p];
    if (flag[p]) src[pos[p]] = (int)p - first;
  }
}

// the plan: components [0, K) sorted by size; [0, K_glob) global-state, [K_glob, K_big) LDS-state (both 256-thread
// items of spi[c] sources), [K_big, K) one wave each.  ibase / pbase: each component's first item and first partial.
__global__ void __launch_bounds__(kThreads) bt_plan_kernel(const int *csize, const int *cstart, const unsigned *rstart,
                                                           size_t n, int small_max, int lds_max, int k_src, int *spi,
                                                           int *ibase, long long *pbase, long long *hdr) {
  __shared__ long long s_part[kThreads], s_items[kThreads];
  __shared__ double s_work[kThreads];
  __shared__ int s_k[kThreads], s_big[kThreads], s_glob[kThreads], s_k4[kThreads];
  __shared__ long long s_adj[kThreads];
  const int tid = threadIdx.x;
  int k = 0, kb = 0, kg = 0, k4 = 0;
  long long adj_sum = 0;
  double work = 0;
  for (size_t c = tid; c < n; c += kThreads) {
    const int nc = csize[c];
    if (nc == 0) continue;
    ++k;
    if (nc > 3) ++k4;
    const long long adj = (long long)rstart[cstart[c + 1]] - rstart[cstart[c]];
    adj_sum += adj;
    if (nc > small_max) {
      ++kb;
      work += (double)(nc < k_src ? nc : k_src) * (double)(adj + nc);
      if (nc > lds_max) ++kg;
    }
  }
  s_k[tid] = k;
  s_big[tid] = kb;
  s_glob[tid] = kg;
  s_k4[tid] = k4;
  s_work[tid] = work;
  s_adj[tid] = adj_sum;
  __syncthreads();
  if (tid == 0) {
    int K = 0, KB = 0, KG = 0, K4 = 0;
    double W = 0;
    long long A = 0;
    for (int q = 0; q < kThreads; ++q) {
      K += s_k[q];
      KB += s_big[q];
      KG += s_glob[q];
      K4 += s_k4[q];
      W += s_work[q];
      A += s_adj[q];
    }
    s_k[0] = K;
    s_big[0] = KB;
    s_glob[0] = KG;
    s_work[0] = W;
    hdr[H_K] = K;
    hdr[H_KBIG] = KB;
    hdr[H_KGLOB] = KG;
    hdr[H_K4] = K4;                // the components of more than 3 vertices: the summary's (a prefix: sorted by size)
    hdr[H_WORK] = (long long)W;    // sum of sources (adjacency + nc) over the 256-thread components (measurement)
    hdr[H_ADJ] = A;
  }
  __syncthreads();
  const int K = s_k[0], KB = s_big[0], KG = s_glob[0];
  const double target = s_work[0] / kBtItems > 1.0 ? s_work[0] / kBtItems : 1.0;
  // per-thread contiguous ranges of components, then one scan of the 256 sums
  const int per = (K + kThreads - 1) / kThreads, c0 = tid * per, c1 = c0 + per < K ? c0 + per : K;
  long long items = 0, part = 0;
  for (int c = c0; c < c1; ++c) {
    const int nc = csize[c], nsrc = nc < k_src ? nc : k_src;
    int s = nsrc;
    if (c < KB) {
      const double cost = (double)((long long)rstart[cstart[c + 1]] - rstart[cstart[c]] + nc);
      const double want = ceil(target / cost);
      s = want < (double)nsrc ? (int)want : nsrc;
      if (s < 1) s = 1;
    }
    spi[c] = s;
    const int it = (nsrc + s - 1) / s;
    items += it;
    part += (long long)it * nc;
  }
  s_items[tid] = items;
  s_part[tid] = part;
  __syncthreads();
  if (tid == 0) {
    long long ri = 0, rp = 0;
    for (int q = 0; q < kThreads; ++q) {
      const long long a = s_items[q], b = s_part[q];
      s_items[q] = ri;
      s_part[q] = rp;
      ri += a;
      rp += b;
    }
    ibase[K] = (int)ri;
    pbase[K] = rp;
    hdr[H_PARTIAL] = rp;
  }
  __syncthreads();
  items = s_items[tid];
  part = s_part[tid];
  for (int c = c0; c < c1; ++c) {
    const int nc = csize[c], it = ((nc < k_src ? nc : k_src) + spi[c] - 1) / spi[c];
    ibase[c] = (int)items;
    pbase[c] = part;
    items += it;
    part += (long long)it * nc;
  }
  __syncthreads();
  if (tid == 0) {
    hdr[H_ITEMS] = ibase[KB];
    hdr[H_ITEMS_GLOB] = ibase[KG];
    hdr[H_NC_GLOB] = KG > 0 ? csize[0] : 0;
    hdr[H_NC_LDS] = KG < KB ? csize[KG] : 0;
  }
}

// Brandes for sources [s0, s1) of one component of nc vertices -- the ids themselves, or with a source list (a sampled
// component) src[s0 .. s1) -- (comp-relative ids; the local CSR row of v is
// rstart[base + v] ..., its neighbours nb[] - base).  SUB lanes share a vertex (64: a wave walks the row; 1: a lane).
// State: lev / q (BFS order) / ls (level starts, nc + 2) int, sig (path counts), cof = (1 + delta) / sig and bc (this
// item's sum over its sources) double.  Levels are pushed (discover), sigma and delta pulled in CSR order, so every
// value is a fixed-order sum whatever order the queue was filled in.
template <int SUB>
__device__ __forceinline__ double bt_sum(double x) {
  if (SUB > 1)
#pragma unroll
    for (int o = SUB / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, SUB);
  return x;
}

template <int SUB>
__device__ __forceinline__ void bt_brandes(const unsigned *__restrict__ rstart, const int *__restrict__ nb, int base,
                                           int nc, int s0, int s1, const int *__restrict__ src, int *lev, int *q, int *ls,
                                           double *sig, double *cof, double *bc, int *tail) {
  const int tid = threadIdx.x, nthr = blockDim.x, g = tid / SUB, l = tid % SUB, ng = nthr / SUB;
  const unsigned *rs = rstart + base;
  for (int v = tid; v < nc; v += nthr) bc[v] = 0.0;
  for (int si = s0; si < s1; ++si) {
    const int s = src ? src[si] : si;
    for (int v = tid; v < nc; v += nthr) lev[v] = -1;
    __syncthreads();
    if (tid == 0) {
      lev[s] = 0;
      sig[s] = 1.0;
      q[0] = s;
      ls[0] = 0;
      ls[1] = 1;
      *tail = 1;
    }
    __syncthreads();
    int d = 0;
    while (true) {                       // level d: its sigma (pulled from d - 1), and level d + 1 discovered
      const int a = ls[d], b = ls[d + 1];
      if (a == b) break;
      for (int k = a + g; k < b; k += ng) {
        const int w = q[k];
        double acc = 0.0;
        for (unsigned e = rs[w] + l; e < rs[w + 1]; e += SUB) {
          const int x = nb[e] - base;
          const int lx = lev[x];
          if (lx < 0) {                  // (before the sigma test: at d = 0, d - 1 is the undiscovered mark)
            if (atomicCAS(&lev[x], -1, d + 1) == -1) q[atomicAdd(tail, 1)] = x;
          } else if (lx == d - 1) {
            acc += sig[x];
          }
        }
        acc = bt_sum<SUB>(acc);
        if (d > 0 && l == 0) sig[w] = acc;
      }
      __syncthreads();
      if (tid == 0) ls[d + 2] = *tail;
      __syncthreads();
      ++d;
    }
    for (int dd = d - 1; dd >= 1; --dd) {    // levels d - 1 .. 1: delta pulled from the level below
      const int a = ls[dd], b = ls[dd + 1];
      for (int k = a + g; k < b; k += ng) {
        const int v = q[k];
        double acc = 0.0;
        for (unsigned e = rs[v] + l; e < rs[v + 1]; e += SUB) {
          const int x = nb[e] - base;
          if (lev[x] == dd + 1) acc += cof[x];
        }
        acc = bt_sum<SUB>(acc);
        if (l == 0) {
          const double sv = sig[v], delta = sv * acc;
          bc[v] += delta;
          cof[v] = (1.0 + delta) / sv;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int bt_comp_of(const int *first, int count, int x) {   // last c < count with first[c] <= x
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// 256-thread items [i0, i1) (dynamic fetch: which workgroup runs an item changes nothing it writes); state in LDS
// (slab == nullptr) or in this workgroup's part of a global slab of slab_stride bytes
template <bool IN_LDS>
__global__ void __launch_bounds__(kThreads) bt_items_kernel(const unsigned *rstart, const int *nb, const int *csize,
                                                            const int *cstart, const int *spi, const int *ibase,
                                                            const long long *pbase, const int *src, const int *sbase,
                                                            int k_src, int kbig, int i0, int i1, unsigned *next,
                                                            char *slab, size_t slab_stride, double *partial) {
  extern __shared__ double lds_state[];
  __shared__ int item, tail;
  char *mine = IN_LDS ? reinterpret_cast<char *>(lds_state) : slab + (size_t)blockIdx.x * slab_stride;
  while (true) {
    __syncthreads();
    if (threadIdx.x == 0) item = i0 + (int)atomicAdd(next, 1u);
    __syncthreads();
    const int k = item;
    if (k >= i1) break;
    const int c = bt_comp_of(ibase, kbig, k), nc = csize[c], base = cstart[c];
    const int nsrc = nc < k_src ? nc : k_src;
    const int s0 = (k - ibase[c]) * spi[c], s1 = s0 + spi[c] < nsrc ? s0 + spi[c] : nsrc;
    double *sig = reinterpret_cast<double *>(mine), *cof = sig + nc, *bc = cof + nc;
    int *lev = reinterpret_cast<int *>(bc + nc), *q = lev + nc, *ls = q + nc;
    bt_brandes<64>(rstart, nb, base, nc, s0, s1, nc > k_src ? src + sbase[c] : nullptr, lev, q, ls, sig, cof, bc, &tail);
    __syncthreads();
    double *out = partial + pbase[c] + (long long)(k - ibase[c]) * nc;
    for (int v = threadIdx.x; v < nc; v += blockDim.x) out[v] = bc[v];
  }
}

// one wave per component of at most kBtSmallCap vertices, every source (or the k_src of its list)
__global__ void __launch_bounds__(64) bt_small_kernel(const unsigned *rstart, const int *nb, const int *csize,
                                                      const int *cstart, const long long *pbase, const int *src,
                                                      const int *sbase, int k_src, int k0, double *partial) {
  __shared__ double sig[kBtSmallCap], cof[kBtSmallCap], bc[kBtSmallCap];
  __shared__ int lev[kBtSmallCap], q[kBtSmallCap], ls[kBtSmallCap + 2], tail;
  const int c = k0 + blockIdx.x, nc = csize[c];
  if (nc > kBtSmallCap) return;        // (the plan never sends one)
  bt_brandes<1>(rstart, nb, cstart[c], nc, 0, nc < k_src ? nc : k_src, nc > k_src ? src + sbase[c] : nullptr, lev, q, ls,
                sig, cof, bc, &tail);
  __syncthreads();
  double *out = partial + pbase[c];
  for (int v = threadIdx.x; v < nc; v += blockDim.x) out[v] = bc[v];
}

// per scored vertex: the sum of its component's partials in item order, over (nc - 1)(nc - 2).  A division, not a
// product with the rounded reciprocal: a sum that is exact (a star's centre, (nc - 1)(nc - 2) itself) gives the
// correctly rounded value, 1.0, where x * (1 / x) falls one ulp short for 50 of the sizes below 400 (nc = 301 is one).
// A sampled component (nc > k_src): (sum * nc) / (k_src * ((nc - 1)(nc - 2))).  wval (whole-graph calls): the same two
// forms with (n_all - 1)(n_all - 2) as the product, n_all = the graph's vertex count.
__global__ void __launch_bounds__(kThreads) bt_reduce_kernel(const double *partial, const int *csize,
                                                             const int *cstart, const int *ibase,
                                                             const long long *pbase, const long long *hdr, int k_src,
                                                             long long n_all, double *val, double *wval) {
  const int K = (int)hdr[H_K], ns = (int)hdr[H_SCORED];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < ns; p += gridDim.x * blockDim.x) {
    const int c = bt_comp_of(cstart, K, p), nc = csize[c], items = ibase[c + 1] - ibase[c];
    const double *x = partial + pbase[c] + (p - cstart[c]);
    double acc = 0.0;
    for (int k = 0; k < items; ++k) acc += x[(long long)k * nc];
    const double own = (double)(nc - 1) * (double)(nc - 2), all = (double)(n_all - 1) * (double)(n_all - 2);
    if (nc > k_src) {
      const double num = acc * (double)nc;
      val[p] = num / ((double)k_src * own);
      if (wval) wval[p] = num / ((double)k_src * all);
    } else {
      val[p] = acc / own;
      if (wval) wval[p] = acc / all;
    }
  }
}

// per component its maximum; then (one thread, component order) the mean and the size-weighted mean
__global__ void __launch_bounds__(kThreads) bt_summary_kernel(const double *val, const int *csize, const int *cstart,
                                                              const long long *hdr, double *cmax, int t, double *bt,
                                                              long long *scored) {
  const int K = (int)hdr[H_K4];
  for (int c = threadIdx.x; c < K; c += blockDim.x) {
    double m = 0.0;
    for (int p = cstart[c]; p < cstart[c + 1]; ++p) m = val[p] > m ? val[p] : m;
    cmax[c] = m;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double mean = 0.0, wmean = 0.0;
  if (K == 1) {
    mean = wmean = cmax[0];
  } else if (K > 1) {
    double s = 0.0, sw = 0.0, w = 0.0;
    for (int c = 0; c < K; ++c) {
      s += cmax[c];
      sw += cmax[c] * (double)csize[c];
      w += (double)csize[c];
    }
    mean = s / K;
    wmean = sw / w;
  }
  bt[2 * t] = mean;
  bt[2 * t + 1] = wmean;
  if (scored) scored[t] = K;
}

__global__ void __launch_bounds__(kThreads) bt_values_kernel(const double *val, const int *order, const long long *hdr,
                                                             double *values) {
  const int ns = (int)hdr[H_SCORED];
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < ns; p += gridDim.x * blockDim.x) values[order[p]] = val[p];
}

// offsets without edges of their own repeat the row before them (zeros before the first edge)
__global__ void bt_fill_kernel(const unsigned *cnt, int n_off, double *bt, long long *scored) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int t = 0; t < n_off; ++t) {
    if (cnt[t]) continue;
    bt[2 * t] = t ? bt[2 * t - 2] : 0.0;
    bt[2 * t + 1] = t ? bt[2 * t - 1] : 0.0;
    if (scored) scored[t] = t ? scored[t - 1] : 0;
  }
}

// what the betweenness stage reads from the counts' stages, and writes
struct BtJob {
  double *bt;                  // [n_off][2]
  long long *scored;           // [n_off] or nullptr
  double *values;              // [n] or nullptr
  long long values_at;         // -1: no values
  int k_src;                   // sources per component at most (INT_MAX: every vertex, ppk_network_summary)
  unsigned long long seed;     // ... of the sample
  bool whole;                  // values: every component of >= 3 vertices, normalised by the whole graph's size
};

int bt_run(const BtJob &job, hipStream_t s, int dev, size_t n, size_t m, size_t no, const std::vector<unsigned> &counts,
           const std::vector<unsigned> &starts, const unsigned *cnt, const int *bu, const int *bv, int *parent,
           const unsigned long long *keys, const int *nbr) {
  const size_t e = 2 * m;
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < n) ++bits;
  const unsigned end_bit = 32 + bits;
  size_t sort_tmp = 0, sort_tmp2 = 0;
  if (n) PPK_HIP(rocprim::radix_sort_keys(nullptr, sort_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr, n, 0u, end_bit, s));
  if (e) PPK_HIP(rocprim::radix_sort_keys(nullptr, sort_tmp2, (unsigned long long *)nullptr, (unsigned long long *)nullptr, e, 0u, end_bit, s));
  size_t tmp = sort_tmp > sort_tmp2 ? sort_tmp : sort_tmp2;
  // a sampled call's source lists (bt_sources) and a whole-graph call's second normalisation: no bytes otherwise
  const bool sampled = job.k_src != INT_MAX;
  const int min_nc = job.whole ? 3 : 4;
  const size_t n_s = sampled ? n : 0, n_w = job.whole ? n : 0;
  if (n_s) {
    size_t pair_tmp = 0, scan_tmp = 0;
    PPK_HIP(rocprim::radix_sort_pairs(nullptr, pair_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                      (int *)nullptr, (int *)nullptr, n, 0u, end_bit, s));
    PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, (int *)nullptr, (int *)nullptr, 0, n, rocprim::plus<int>(), s));
    tmp = tmp > pair_tmp ? tmp : pair_tmp;
    tmp = tmp > scan_tmp ? tmp : scan_tmp;
  }
  long long *hdr, *pbase;
  unsigned *fill, *rstart;
  int *root, *size, *crank, *csize, *cstart, *spi, *ibase, *local, *order, *lnbr;
  int *sid_a, *sid_b, *sflag, *spos, *src, *sbase;
  unsigned long long *ka, *kb, *ea, *eb, *ska, *skb;
  double *val, *cmax, *wval;
  char *d_tmp;
  int rc = ppk_scratch_carve(dev, SLOT_NET_BT, [&](Carve &c) {
    c.take(hdr, H_LEN).take(fill, 1).take(root, n).take(size, n).take(crank, n);
    c.take(csize, n + 2).take(cstart, n + 2).take(spi, n + 2).take(ibase, n + 2).take(pbase, n + 2);
    c.take(local, n).take(order, n).take(ka, n).take(kb, n).take(rstart, n + 1).take(val, n).take(cmax, n);
    c.take(ea, e).take(eb, e).take(lnbr, e).take(d_tmp, tmp + 16);
    c.take(ska, n_s).take(skb, n_s).take(sid_a, n_s).take(sid_b, n_s).take(sflag, n_s).take(spos, n_s);
    c.take(src, n_s).take(sbase, n_s ? n + 2 : 0).take(wval, n_w);
  });
  if (rc != PPK_OK) return rc;
  if (!job.whole) wval = nullptr;

  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  const bool big_lds = ppk_lds_opt_in(reinterpret_cast<const void *>(bt_items_kernel<true>), dev, (int)kBtLdsBytes);
  long long lds_max = (long long)(((big_lds ? kBtLdsBytes : 65536 - 64) - 8) / 36);
  const long long forced_lds = ppk_config().bt_lds_max.load();
  if (forced_lds > 0 && forced_lds < lds_max) lds_max = forced_lds;
  long long small_max = ppk_config().bt_small_max.load();
  if (small_max < 0) small_max = 0;
  if (small_max > kBtSmallCap) small_max = kBtSmallCap;

  // the graph values are read from: the last one at or before values_at that adds edges
  long long values_graph = -1;
  if (job.values) {
    PPK_HIP(hipMemsetAsync(job.values, 0, n * 8, s));
    for (long long o = 0; o <= job.values_at && o < (long long)no; ++o)
      if (counts[o]) values_graph = o;
  }

  hipLaunchKernelGGL(net_parent_init_kernel, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, s, parent, n);
  PPK_HIP(hipGetLastError());
  size_t edges_t = 0;
  for (size_t o = 0; o < no; ++o) {
    if (!counts[o]) continue;
    edges_t += counts[o];
    // -- relabel
    ppk_prof_stage("bt_relabel", s);
    hipLaunchKernelGGL(net_union_kernel, dim3(grid_for(counts[o], kThreads * 4, 2048)), dim3(kThreads), 0, s,
                       bu + starts[o], bv + starts[o], counts[o], parent, fill + 1);
    PPK_HIP(hipMemsetAsync(size, 0, n * 4, s));
    PPK_HIP(hipMemsetAsync(fill, 0, 4, s));
    const dim3 gn(grid_for(n, kThreads, 4096));
    hipLaunchKernelGGL(bt_sizes_kernel, gn, dim3(kThreads), 0, s, parent, n, root, size);
    hipLaunchKernelGGL(bt_root_keys_kernel, gn, dim3(kThreads), 0, s, root, size, n, min_nc, ka);
    size_t tb = tmp;
    PPK_HIP(rocprim::radix_sort_keys(d_tmp, tb, ka, kb, n, 0u, end_bit, s));
    hipLaunchKernelGGL(bt_comps_kernel, dim3(grid_for(n + 1, kThreads, 4096)), dim3(kThreads), 0, s, kb, size, n,
                       crank, csize);
    hipLaunchKernelGGL(bt_starts_kernel, dim3(1), dim3(kThreads), 0, s, csize, n, cstart, hdr);
    hipLaunchKernelGGL(bt_vertex_keys_kernel, gn, dim3(kThreads), 0, s, root, size, crank, n, min_nc, ka,
                       local);
    tb = tmp;
    PPK_HIP(rocprim::radix_sort_keys(d_tmp, tb, ka, kb, n, 0u, end_bit, s));
    hipLaunchKernelGGL(bt_local_kernel, gn, dim3(kThreads), 0, s, kb, n, local, order);
    const size_t len = 2 * edges_t;
    PPK_HIP(hipMemsetAsync(ea, 0xff, len * 8, s));
    hipLaunchKernelGGL(bt_edges_kernel, dim3(grid_for(e, kThreads * 8, 4096)), dim3(kThreads), 0, s, keys, nbr, e,
                       (unsigned)o, local, fill, ea);
    tb = tmp;
    PPK_HIP(rocprim::radix_sort_keys(d_tmp, tb, ea, eb, len, 0u, end_bit, s));
    hipLaunchKernelGGL(bt_rows_kernel, dim3(grid_for(len, kThreads, 8192)), dim3(kThreads), 0, s, eb, len, hdr,
                       rstart, lnbr);
    PPK_HIP(hipGetLastError());
    if (sampled) {
      // -- sources: (component, sample key) sorted over the local ids; the first k of each larger component, listed
      ppk_prof_stage("bt_sources", s);
      hipLaunchKernelGGL(bt_src_keys_kernel, gn, dim3(kThreads), 0, s, kb, csize, hdr, n, job.k_src, job.seed, ska,
                         sid_a, sflag);
      tb = tmp;
      PPK_HIP(rocprim::radix_sort_pairs(d_tmp, tb, ska, skb, sid_a, sid_b, n, 0u, end_bit, s));
      hipLaunchKernelGGL(bt_src_pick_kernel, gn, dim3(kThreads), 0, s, skb, sid_b, csize, cstart, hdr, job.k_src, sflag);
      tb = tmp;
      PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, sflag, spos, 0, n, rocprim::plus<int>(), s));
      hipLaunchKernelGGL(bt_src_list_kernel, gn, dim3(kThreads), 0, s, kb, sflag, spos, cstart, hdr, src, sbase);
      PPK_HIP(hipGetLastError());
    }
    // -- plan: the graph's one synchronisation
    ppk_prof_stage("bt_plan", s);
    hipLaunchKernelGGL(bt_plan_kernel, dim3(1), dim3(kThreads), 0, s, csize, cstart, rstart, n, (int)small_max,
                       (int)lds_max, job.k_src, spi, ibase, pbase, hdr);
    PPK_HIP(hipGetLastError());
    const unsigned long long *h = nullptr;
    if ((rc = ppk_read_back(dev, s, {{hdr, H_LEN * 8}}, &h)) != PPK_OK) return rc;
    const int K = (int)h[H_K], kbig = (int)h[H_KBIG], n_items = (int)h[H_ITEMS], items_glob = (int)h[H_ITEMS_GLOB];
    const size_t n_partial = (size_t)h[H_PARTIAL], nc_glob = (size_t)h[H_NC_GLOB], nc_lds = (size_t)h[H_NC_LDS];
    // -- Brandes
    ppk_prof_stage("bt_brandes", s);
    if (K > 0) {
      const unsigned g_glob = items_glob > 0 ? (unsigned)(items_glob < 2 * cus ? items_glob : 2 * cus) : 0;
      const size_t slab_stride = align256(bt_state_bytes(nc_glob));
      unsigned *next;
      double *partial;
      char *slab;
      rc = ppk_scratch_carve(dev, SLOT_NET_WORK, [&](Carve &c) {
        c.take(next, 2).take(partial, n_partial).take(slab, g_glob * slab_stride);
      });
      if (rc != PPK_OK) return rc;
      PPK_HIP(hipMemsetAsync(next, 0, 8, s));
      if (items_glob > 0)
        hipLaunchKernelGGL(bt_items_kernel<false>, dim3(g_glob), dim3(kThreads), 0, s, rstart, lnbr, csize, cstart,
                           spi, ibase, pbase, src, sbase, job.k_src, kbig, 0, items_glob, next, slab, slab_stride,
                           partial);
      if (n_items > items_glob) {
        const int li = n_items - items_glob;
        hipLaunchKernelGGL(bt_items_kernel<true>, dim3((unsigned)(li < 8 * cus ? li : 8 * cus)), dim3(kThreads),
                           bt_state_bytes(nc_lds), s, rstart, lnbr, csize, cstart, spi, ibase, pbase, src, sbase,
                           job.k_src, kbig, items_glob, n_items, next + 1, (char *)nullptr, (size_t)0, partial);
      }
      if (K > kbig)
        hipLaunchKernelGGL(bt_small_kernel, dim3((unsigned)(K - kbig)), dim3(64), 0, s, rstart, lnbr, csize, cstart,
                           pbase, src, sbase, job.k_src, kbig, partial);
      PPK_HIP(hipGetLastError());
      ppk_prof_stage("bt_reduce", s);
      hipLaunchKernelGGL(bt_reduce_kernel, dim3(grid_for((size_t)h[H_SCORED], kThreads, 4096)), dim3(kThreads), 0, s,
                         partial, csize, cstart, ibase, pbase, hdr, job.k_src, (long long)n, val, wval);
    }
    if (K == 0) ppk_prof_stage("bt_reduce", s);
    hipLaunchKernelGGL(bt_summary_kernel, dim3(1), dim3(kThreads), 0, s, val, csize, cstart, hdr, cmax, (int)o, job.bt,
                       job.scored);
    if ((long long)o == values_graph && K > 0)
      hipLaunchKernelGGL(bt_values_kernel, dim3(grid_for((size_t)h[H_SCORED], kThreads, 4096)), dim3(kThreads), 0, s,
                         job.whole ? wval : val, order, hdr, job.values);
    PPK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(bt_fill_kernel, dim3(1), dim3(64), 0, s, cnt, (int)no, job.bt, job.scored);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

// the sizes of a host-array network call, checked (who: the entry point's name)
int net_check(const std::string &who, size_t n_edges, size_t n_vertices, size_t n_off) {
  if (n_off == 0 || n_off > (size_t)kMaxOff) return ppk_fail(PPK_ERR_ARG, who + ": n_off must be 1 .. 1023");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_edges must be < 2^31");
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_vertices must be < 2^31");
  return PPK_OK;
}

int net_sweep(const std::string &who, const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
              size_t n_edges, size_t n_vertices, size_t n_off, long long labels_at, long long *d_stats,
              int32_t *d_labels, void *stream, const BtJob *bt) {
  if (n_off == 0 || n_off > (size_t)kMaxOff) return ppk_fail(PPK_ERR_ARG, who + ": n_off must be 1 .. 1023");
  if (!d_off && n_off != 1 && n_edges) return ppk_fail(PPK_ERR_ARG, who + ": no offset array needs n_off == 1");
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_vertices must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_edges must be < 2^31");
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, who + ": stride must be 1 or 2");
  if (labels_at < -1 || labels_at >= (long long)n_off)
    return ppk_fail(PPK_ERR_ARG, who + ": labels_at must be -1 or an offset index");
  if (!d_stats || (labels_at >= 0 && !d_labels && n_vertices) || (n_edges && (!d_i || !d_j)))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
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
  unsigned long long *bad, *tri, *wed, *ka, *kb;
  unsigned *cnt, *cursor, *links, *start2;
  int *parent, *is_root, *rank, *bu, *bv, *va, *vb;
  uint16_t *off16;
  char *d_tmp;
  size_t zero_begin = 0, zero_end = 0;
  int rc = ppk_scratch_carve(dev, SLOT_NET, [&](Carve &c) {
    c.take(bad, 1);
    zero_begin = c.at;
    c.take(cnt, 1024).take(cursor, 1024).take(links, 1024).take(tri, 1024).take(wed, 1024);
    zero_end = c.at;
    c.take(parent, n).take(is_root, n).take(rank, n).take(start2, 2 * n + 1).take(bu, m).take(bv, m);
    c.take(ka, e).take(kb, e).take(va, e).take(vb, e).take(off16, e).take(d_tmp, tmp + 16);
  });
  if (rc != PPK_OK) return rc;

  // -- validate: the one synchronisation
  ppk_prof_stage("validate", s);
  PPK_HIP(hipMemsetAsync(cnt, 0, zero_end - zero_begin, s));
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  const unsigned cap_grid = 2048;
  if (m)
    hipLaunchKernelGGL(net_validate_kernel, dim3(grid_for(m, kThreads * 8, cap_grid)), dim3(kThreads), 0, s, d_i, d_j,
                       stride, d_off, m, (long long)n, (int)no, cnt, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 8}, {cnt, no * 4}}, &h)) != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return bad_edge_message(who, d_i, d_j, stride, d_off, (size_t)h[0], n, no);
  }
  std::vector<unsigned> counts(no), starts(no);
  memcpy(counts.data(), h + 1, no * 4);     // before bt_run's read-back reuses the block
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
    const unsigned tl = table_entries(n, ppk_lds_opt_in(reinterpret_cast<const void *>(net_triangles_kernel), dev,
                                                        (int)(kTableMax * sizeof(uint16_t))));
    hipLaunchKernelGGL(net_triangles_kernel, dim3((unsigned)(n < (1u << 20) ? n : (1u << 20))), dim3(kThreads),
                       tl * sizeof(uint16_t), s, nbr, off16, start2, n, (int)no, tl, tri);
    PPK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(net_stats_kernel, dim3(1), dim3(64), 0, s, cnt, links, tri, wed, (long long)n, (int)no, d_stats);
  if (bt) {
    PPK_HIP(hipGetLastError());
    rc = bt_run(*bt, s, dev, n, m, no, counts, starts, cnt, bu, bv, parent, kb, nbr);
    if (rc != PPK_OK) {
      ppk_prof_stage(nullptr, s);
      return rc;
    }
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

// ---- cluster numbers of every G_t ---------------------------------------------------------------
// The validate stage and the buckets are the sweep's; after every union launch that changed the forest:
//   clu_sizes    bt_sizes_kernel: every vertex's root, every root's size (integer atomics)
//   clu_rank     one key per root, (n - size, n - 1 - root): ascending order = size descending, then root descending,
//                which is len - rankdata(sizes, 'ordinal') over components taken in the order of their smallest
//                vertex (a root IS the smallest vertex of its set); rocPRIM radix sort; position + 1 is the number
//   clu_scatter  row t: every vertex reads its root's number
// An offset without edges of its own copies the row before it; offset 0 is always computed (no edges: all singletons,
// n - v).  n_clusters[t] = n - the links so far.
// Seeded (ppk_cluster_extend_dev): vertices 0 .. n_ref-1 arrive as components, label[r] in [0, n_ref).
//   clu_seed_first  first[l] = the smallest r with label[r] == l (atomicMin); a label out of range is the bad reference
//   clu_seed        parent[r] = first[label[r]], parent[v >= n_ref] = v: parent[x] <= x and a root is its set's smallest
//                   vertex, which is all uf_union and the ranking ask; every non-root counts as a link at offset 0
// and the rest is the unseeded call's, over the new edges alone.
__global__ void __launch_bounds__(kThreads) clu_seed_first_kernel(const int32_t *label, size_t n_ref, unsigned *first,
                                                                  unsigned long long *bad) {
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_ref; r += (size_t)gridDim.x * blockDim.x) {
    const long long l = label[r];
    if (l < 0 || l >= (long long)n_ref) atomicMin(bad, (unsigned long long)r);
    else atomicMin(&first[l], (unsigned)r);
  }
}
__global__ void __launch_bounds__(kThreads) clu_seed_kernel(const int32_t *label, const unsigned *first, size_t n_ref,
                                                            size_t n, int *parent, unsigned *links0) {
  unsigned mine = 0;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const int p = v < n_ref ? (int)first[label[v]] : (int)v;
    parent[v] = p;
    mine += p != (int)v;
  }
  __shared__ unsigned acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  if (mine) atomicAdd(&acc, mine);
  __syncthreads();
  const unsigned tot = acc;
  if (threadIdx.x == 0 && tot) atomicAdd(links0, tot);
}
__global__ void __launch_bounds__(kThreads) clu_root_keys_kernel(const int *root, const int *size, size_t n,
                                                                 unsigned long long *keys) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    keys[v] = root[v] == (int)v ? ((unsigned long long)(n - size[v]) << 32 | (unsigned long long)(n - 1 - v)) : kNone;
}
__global__ void __launch_bounds__(kThreads) clu_numbers_kernel(const unsigned long long *sorted, size_t n, int *number) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = sorted[p];
    if (key != kNone) number[n - 1 - (size_t)(key & 0xffffffffu)] = (int)(p + 1);
  }
}
__global__ void __launch_bounds__(kThreads) clu_scatter_kernel(const int *root, const int *number, size_t n,
                                                               int32_t *row) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    row[v] = number[root[v]];
}
__global__ void clu_counts_kernel(const unsigned *links, long long n, int n_off, int32_t *n_clusters) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long l = 0;
  for (int o = 0; o < n_off; ++o) {
    l += links[o];
    n_clusters[o] = (int32_t)(n - l);
  }
}

int cluster_sweep(const std::string &who, const long long *d_i, const long long *d_j, size_t stride,
                  const long long *d_off, size_t n_edges, size_t n_vertices, size_t n_off, int32_t *d_clusters,
                  int32_t *d_n_clusters, void *stream, const int32_t *d_ref_label = nullptr, size_t n_ref = 0) {
  if (n_off == 0 || n_off > (size_t)kMaxOff) return ppk_fail(PPK_ERR_ARG, who + ": n_off must be 1 .. 1023");
  if (!d_off && n_off != 1 && n_edges) return ppk_fail(PPK_ERR_ARG, who + ": no offset array needs n_off == 1");
  if (n_vertices >= ((size_t)1 << 31))
    return ppk_fail(PPK_ERR_ARG, who + (d_ref_label ? ": n_ref + n_qry must be < 2^31" : ": n_vertices must be < 2^31"));
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_edges must be < 2^31");
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, who + ": stride must be 1 or 2");
  if (!d_n_clusters || (!d_clusters && n_vertices) || (n_edges && (!d_i || !d_j)))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n_edges, n = n_vertices, no = n_off;

  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) < n) ++bits;
  const unsigned end_bit = 32 + bits + 1;      // n - size < 2^bits: kNone sorts after every root's key
  size_t sort_tmp = 0, scan_tmp = 0;
  if (n) PPK_HIP(rocprim::radix_sort_keys(nullptr, sort_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr, n, 0u, end_bit, s));
  PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, (unsigned *)nullptr, (unsigned *)nullptr, 0u, no,
                                  rocprim::plus<unsigned>(), s));
  const size_t tmp = sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
  unsigned long long *bad, *ka, *kb;
  unsigned *cnt, *cursor, *links, *first;
  int *parent, *root, *size, *number, *bu, *bv;
  char *d_tmp;
  size_t zero_begin = 0, zero_end = 0;
  int rc = ppk_scratch_carve(dev, SLOT_NET, [&](Carve &c) {
    c.take(bad, 2);                      // the first bad edge, the first bad reference label
    zero_begin = c.at;
    c.take(cnt, 1024).take(cursor, 1024).take(links, 1024);
    zero_end = c.at;
    c.take(parent, n).take(root, n).take(size, n).take(number, n).take(bu, m).take(bv, m);
    c.take(ka, n).take(kb, n).take(first, n_ref).take(d_tmp, tmp + 16);
  });
  if (rc != PPK_OK) return rc;

  // -- validate: the one synchronisation
  ppk_prof_stage("validate", s);
  PPK_HIP(hipMemsetAsync(cnt, 0, zero_end - zero_begin, s));
  PPK_HIP(hipMemsetAsync(bad, 0xff, 16, s));
  if (n_ref) {
    PPK_HIP(hipMemsetAsync(first, 0xff, n_ref * 4, s));
    hipLaunchKernelGGL(clu_seed_first_kernel, dim3(grid_for(n_ref, kThreads * 4, 2048)), dim3(kThreads), 0, s,
                       d_ref_label, n_ref, first, bad + 1);
  }
  if (m)
    hipLaunchKernelGGL(net_validate_kernel, dim3(grid_for(m, kThreads * 8, 2048)), dim3(kThreads), 0, s, d_i, d_j,
                       stride, d_off, m, (long long)n, (int)no, cnt, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 16}, {cnt, no * 4}}, &h)) != PPK_OK) return rc;
  if (h[1] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    int32_t l = 0;
    PPK_HIP(hipMemcpy(&l, d_ref_label + h[1], 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": reference " + std::to_string(h[1]) + ": label " + std::to_string(l) +
                                     " outside [0, " + std::to_string(n_ref) + ")");
  }
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return bad_edge_message(who, d_i, d_j, stride, d_off, (size_t)h[0], n, no);
  }
  std::vector<unsigned> counts(no), starts(no);
  memcpy(counts.data(), h + 2, no * 4);
  for (size_t o = 0, acc = 0; o < no; ++o) {
    starts[o] = (unsigned)acc;
    acc += counts[o];
  }

  // -- buckets
  ppk_prof_stage("csr", s);
  if (m) {
    size_t tb = tmp;
    PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, cnt, cursor, 0u, no, rocprim::plus<unsigned>(), s));
    hipLaunchKernelGGL(net_scatter_kernel, dim3(grid_for(m, (size_t)kThreads * kScatterItems, 4096)), dim3(kThreads), 0,
                       s, d_i, d_j, stride, d_off, m, (int)no, cursor, bu, bv, (unsigned long long *)nullptr,
                       (int *)nullptr);
    PPK_HIP(hipGetLastError());
  }

  // -- components and numbers, batch by batch
  ppk_prof_stage("clusters", s);
  if (n) {
    const dim3 gn(grid_for(n, kThreads, 4096));
    if (n_ref) hipLaunchKernelGGL(clu_seed_kernel, gn, dim3(kThreads), 0, s, d_ref_label, first, n_ref, n, parent, links);
    else hipLaunchKernelGGL(net_parent_init_kernel, gn, dim3(kThreads), 0, s, parent, n);
    for (size_t o = 0; o < no; ++o) {
      int32_t *row = d_clusters + o * n;
      if (!counts[o] && o) {
        PPK_HIP(hipMemcpyAsync(row, row - n, n * 4, hipMemcpyDeviceToDevice, s));
        continue;
      }
      if (counts[o])
        hipLaunchKernelGGL(net_union_kernel, dim3(grid_for(counts[o], kThreads * 4, 2048)), dim3(kThreads), 0, s,
                           bu + starts[o], bv + starts[o], counts[o], parent, links + o);
      PPK_HIP(hipMemsetAsync(size, 0, n * 4, s));
      hipLaunchKernelGGL(bt_sizes_kernel, gn, dim3(kThreads), 0, s, parent, n, root, size);
      hipLaunchKernelGGL(clu_root_keys_kernel, gn, dim3(kThreads), 0, s, root, size, n, ka);
      size_t tb = tmp;
      PPK_HIP(rocprim::radix_sort_keys(d_tmp, tb, ka, kb, n, 0u, end_bit, s));
      hipLaunchKernelGGL(clu_numbers_kernel, gn, dim3(kThreads), 0, s, kb, n, number);
      hipLaunchKernelGGL(clu_scatter_kernel, gn, dim3(kThreads), 0, s, root, number, n, row);
      PPK_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(clu_counts_kernel, dim3(1), dim3(64), 0, s, links, (long long)n, (int)no, d_n_clusters);
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_network_sweep_dev(const long long *d_i, const long long *d_j, size_t stride,
                                     const long long *d_off, size_t n_edges, size_t n_vertices, size_t n_off,
                                     long long labels_at, long long *d_stats, int32_t *d_labels, void *stream) {
  return net_sweep("ppk_network_sweep", d_i, d_j, stride, d_off, n_edges, n_vertices, n_off, labels_at, d_stats,
                   d_labels, stream, nullptr);
}

extern "C" int ppk_network_sweep(const long long *i, const long long *j, const long long *off, size_t n_edges,
                                 size_t n_vertices, size_t n_off, int device_id, long long labels_at, long long *stats,
                                 int32_t *labels) {
  if (!stats || (n_edges && (!i || !j)) || (labels_at >= 0 && !labels && n_vertices))
    return ppk_fail(PPK_ERR_ARG, "ppk_network_sweep: NULL array");
  const int rc = net_check("ppk_network_sweep", n_edges, n_vertices, n_off);
  if (rc != PPK_OK) return rc;
  long long *d_i, *d_j, *d_o, *d_stats;
  int32_t *d_labels;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_o, n_edges).take(d_stats, 4 * n_off).take(d_labels, n_vertices);
    c.at += 256;     // (spare)
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
      if (off) PPK_HIP(hipMemcpy(d_o, off, n_edges * 8, hipMemcpyHostToDevice));
    }
    const int rc = ppk_network_sweep_dev(d_i, d_j, 1, off ? d_o : nullptr, n_edges, n_vertices, n_off, labels_at,
                                         d_stats, labels_at >= 0 ? d_labels : nullptr, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(stats, d_stats, n_off * 32, hipMemcpyDeviceToHost));
    if (labels_at >= 0 && n_vertices) PPK_HIP(hipMemcpy(labels, d_labels, n_vertices * 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

namespace {

// ppk_network_summary_dev and its sampled form: k_src = INT_MAX is every source
int summary_dev(const std::string &who, const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
                size_t n_edges, size_t n_vertices, size_t n_off, long long values_at, long long *d_stats, double *d_bt,
                long long *d_scored, double *d_values, int k_src, unsigned long long seed, bool whole, void *stream) {
  if (n_off >= 1 && n_off <= (size_t)kMaxOff && (values_at < -1 || values_at >= (long long)n_off))
    return ppk_fail(PPK_ERR_ARG, who + ": values_at must be -1 or an offset index");
  if (!d_bt || (values_at >= 0 && !d_values && n_vertices)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const BtJob job{d_bt, d_scored, values_at >= 0 && n_vertices ? d_values : nullptr, values_at, k_src, seed, whole};
  return net_sweep(who, d_i, d_j, stride, d_off, n_edges, n_vertices, n_off, -1, d_stats, nullptr, stream, &job);
}

// the sampled calls' own arguments, checked: *k_src = min(bt_sources, INT_MAX)
int sampled_check(const std::string &who, size_t bt_sources, int flags, int *k_src) {
  if (bt_sources == 0) return ppk_fail(PPK_ERR_ARG, who + ": bt_sources must be >= 1");
  if (flags & ~PPK_BT_WHOLE_GRAPH) return ppk_fail(PPK_ERR_ARG, who + ": unknown flag bits");
  *k_src = bt_sources < (size_t)INT_MAX ? (int)bt_sources : INT_MAX;
  return PPK_OK;
}

// the host-array forms: copy in, call `dev_call(d_i, d_j, d_off, d_stats, d_bt, d_scored, d_values)`, copy out
template <typename Call>
int summary_host(const std::string &who, const long long *i, const long long *j, const long long *off, size_t n_edges,
                 size_t n_vertices, size_t n_off, int device_id, long long values_at, long long *stats, double *bt,
                 long long *scored, double *values, Call dev_call) {
  if (!stats || !bt || (n_edges && (!i || !j)) || (values_at >= 0 && !values && n_vertices))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const int rc = net_check(who, n_edges, n_vertices, n_off);
  if (rc != PPK_OK) return rc;
  long long *d_i, *d_j, *d_o, *d_stats, *d_scored;
  double *d_bt, *d_values;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_o, n_edges);
    c.take(d_stats, 4 * n_off).take(d_bt, 2 * n_off).take(d_scored, n_off).take(d_values, n_vertices);
    c.at += 256;     // (spare)
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
      if (off) PPK_HIP(hipMemcpy(d_o, off, n_edges * 8, hipMemcpyHostToDevice));
    }
    const int rc = dev_call(d_i, d_j, off ? d_o : nullptr, d_stats, d_bt, d_scored, values_at >= 0 ? d_values : nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(stats, d_stats, n_off * 32, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(bt, d_bt, n_off * 16, hipMemcpyDeviceToHost));
    if (scored) PPK_HIP(hipMemcpy(scored, d_scored, n_off * 8, hipMemcpyDeviceToHost));
    if (values_at >= 0 && n_vertices) PPK_HIP(hipMemcpy(values, d_values, n_vertices * 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

}  // namespace

extern "C" int ppk_network_summary_dev(const long long *d_i, const long long *d_j, size_t stride,
                                       const long long *d_off, size_t n_edges, size_t n_vertices, size_t n_off,
                                       long long values_at, long long *d_stats, double *d_bt, long long *d_scored,
                                       double *d_values, void *stream) {
  return summary_dev("ppk_network_summary", d_i, d_j, stride, d_off, n_edges, n_vertices, n_off, values_at, d_stats, d_bt,
                     d_scored, d_values, INT_MAX, 0, false, stream);
}

extern "C" int ppk_network_summary(const long long *i, const long long *j, const long long *off, size_t n_edges,
                                   size_t n_vertices, size_t n_off, int device_id, long long values_at, long long *stats,
                                   double *bt, long long *scored, double *values) {
  return summary_host("ppk_network_summary", i, j, off, n_edges, n_vertices, n_off, device_id, values_at, stats, bt,
                      scored, values,
                      [&](const long long *d_i, const long long *d_j, const long long *d_o, long long *d_stats,
                          double *d_bt, long long *d_scored, double *d_values) {
                        return ppk_network_summary_dev(d_i, d_j, 1, d_o, n_edges, n_vertices, n_off, values_at, d_stats,
                                                       d_bt, d_scored, d_values, nullptr);
                      });
}

extern "C" int ppk_network_summary_sampled_dev(const long long *d_i, const long long *d_j, size_t stride,
                                               const long long *d_off, size_t n_edges, size_t n_vertices, size_t n_off,
                                               long long values_at, long long *d_stats, double *d_bt,
                                               long long *d_scored, double *d_values, size_t bt_sources,
                                               unsigned long long seed, int flags, void *stream) {
  int k_src = 0;
  const int rc = sampled_check("ppk_network_summary_sampled", bt_sources, flags, &k_src);
  if (rc != PPK_OK) return rc;
  return summary_dev("ppk_network_summary_sampled", d_i, d_j, stride, d_off, n_edges, n_vertices, n_off, values_at,
                     d_stats, d_bt, d_scored, d_values, k_src, seed, (flags & PPK_BT_WHOLE_GRAPH) != 0, stream);
}

extern "C" int ppk_network_summary_sampled(const long long *i, const long long *j, const long long *off,
                                           size_t n_edges, size_t n_vertices, size_t n_off, int device_id,
                                           long long values_at, long long *stats, double *bt, long long *scored,
                                           double *values, size_t bt_sources, unsigned long long seed, int flags) {
  int k_src = 0;
  const int rc = sampled_check("ppk_network_summary_sampled", bt_sources, flags, &k_src);
  if (rc != PPK_OK) return rc;
  return summary_host("ppk_network_summary_sampled", i, j, off, n_edges, n_vertices, n_off, device_id, values_at, stats,
                      bt, scored, values,
                      [&](const long long *d_i, const long long *d_j, const long long *d_o, long long *d_stats,
                          double *d_bt, long long *d_scored, double *d_values) {
                        return ppk_network_summary_sampled_dev(d_i, d_j, 1, d_o, n_edges, n_vertices, n_off, values_at,
                                                               d_stats, d_bt, d_scored, d_values, bt_sources, seed,
                                                               flags, nullptr);
                      });
}

extern "C" int ppk_cluster_sweep_dev(const long long *d_i, const long long *d_j, size_t stride, const long long *d_off,
                                     size_t n_edges, size_t n_vertices, size_t n_off, int32_t *d_clusters,
                                     int32_t *d_n_clusters, void *stream) {
  return cluster_sweep("ppk_cluster_sweep", d_i, d_j, stride, d_off, n_edges, n_vertices, n_off, d_clusters,
                       d_n_clusters, stream);
}

extern "C" int ppk_cluster_extend_dev(const long long *d_i, const long long *d_j, size_t stride, size_t n_edges,
                                      const int32_t *d_ref_label, size_t n_ref, size_t n_qry, int32_t *d_numbers,
                                      int32_t *d_n_clusters, void *stream) {
  if (n_ref >= ((size_t)1 << 31) || n_qry >= ((size_t)1 << 31) || n_ref + n_qry >= ((size_t)1 << 31))
    return ppk_fail(PPK_ERR_ARG, "ppk_cluster_extend: n_ref + n_qry must be < 2^31");
  if (n_ref && !d_ref_label) return ppk_fail(PPK_ERR_ARG, "ppk_cluster_extend: NULL array");
  return cluster_sweep("ppk_cluster_extend", d_i, d_j, stride, nullptr, n_edges, n_ref + n_qry, 1, d_numbers,
                       d_n_clusters, stream, d_ref_label, n_ref);
}

extern "C" int ppk_cluster_extend(const long long *i, const long long *j, size_t n_edges, const int32_t *ref_label,
                                  size_t n_ref, size_t n_qry, int device_id, int32_t *numbers, int32_t *n_clusters) {
  if (n_ref >= ((size_t)1 << 31) || n_qry >= ((size_t)1 << 31) || n_ref + n_qry >= ((size_t)1 << 31))
    return ppk_fail(PPK_ERR_ARG, "ppk_cluster_extend: n_ref + n_qry must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_cluster_extend: n_edges must be < 2^31");
  if (!n_clusters || (!numbers && n_ref + n_qry) || (n_edges && (!i || !j)) || (n_ref && !ref_label))
    return ppk_fail(PPK_ERR_ARG, "ppk_cluster_extend: NULL array");
  const size_t n = n_ref + n_qry;
  long long *d_i, *d_j;
  int32_t *d_label, *d_numbers, *d_nc;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_label, n_ref).take(d_numbers, n).take(d_nc, 1);
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
    }
    if (n_ref) PPK_HIP(hipMemcpy(d_label, ref_label, n_ref * 4, hipMemcpyHostToDevice));
    const int rc = ppk_cluster_extend_dev(d_i, d_j, 1, n_edges, d_label, n_ref, n_qry, d_numbers, d_nc, nullptr);
    if (rc != PPK_OK) return rc;
    if (n) PPK_HIP(hipMemcpy(numbers, d_numbers, n * 4, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(n_clusters, d_nc, 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" int ppk_cluster_sweep(const long long *i, const long long *j, const long long *off, size_t n_edges,
                                 size_t n_vertices, size_t n_off, int device_id, int32_t *clusters,
                                 int32_t *n_clusters) {
  if (!n_clusters || (!clusters && n_vertices) || (n_edges && (!i || !j)))
    return ppk_fail(PPK_ERR_ARG, "ppk_cluster_sweep: NULL array");
  const int rc = net_check("ppk_cluster_sweep", n_edges, n_vertices, n_off);
  if (rc != PPK_OK) return rc;
  long long *d_i, *d_j, *d_o;
  int32_t *d_clusters, *d_nc;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_o, n_edges).take(d_clusters, n_off * n_vertices).take(d_nc, n_off);
    c.at += 256;     // (spare)
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
      if (off) PPK_HIP(hipMemcpy(d_o, off, n_edges * 8, hipMemcpyHostToDevice));
    }
    const int rc = ppk_cluster_sweep_dev(d_i, d_j, 1, off ? d_o : nullptr, n_edges, n_vertices, n_off, d_clusters,
                                         d_nc, nullptr);
    if (rc != PPK_OK) return rc;
    if (n_vertices) PPK_HIP(hipMemcpy(clusters, d_clusters, n_off * n_vertices * 4, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(n_clusters, d_nc, n_off * 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// Minimum spanning forests and model edge weights on the device.
//
//  - ppk_mst_dev : the minimum spanning forest of a weighted multigraph, for generate_minimum_spanning_tree
//    (PopPUNK/network.py:1721-1831: graph-tool's min_spanning_tree, or cugraph's minimum_spanning_tree).  Edges are
//    totally ordered by (w, min(i, j), max(i, j), input index), so the forest is unique: Kruskal with a stable sort on
//    that key.  Stages (ppk_prof_stages names):
//      validate    one pass checks every id, self-loop and weight; the call's ONE synchronisation reads the first bad
//                  edge
//      rank        two stable rocPRIM radix sorts (min << b | max, then the order-preserving 32-bit key of w): an
//                  edge's position is its rank in the total order; both ends are gathered in rank order
//      boruvka     ceil(log2 n) rounds, each a fixed sequence of launches and no host round trip: every edge between
//                  two roots atomicMin's its rank into both roots' best slot (ranks are unique, so the minimum does
//                  not depend on arrival order); every root hooks along its best edge (a mutual pair: the larger root
//                  hooks under the smaller) and marks that rank; read-only pointer-jumping passes compress the hook
//                  forest, src -> dst, 16 hops a pass.  A word per round (and per pass) written by the launch before
//                  lets every later launch of a finished forest return at once
//      labels      optional: components numbered by their smallest vertex (scipy's connected_components)
//      compact     the marked ranks back to input indices, in ascending input order (rocPRIM select)
//    Kernel boundaries are the only hand-offs between workgroups; the only atomics are integer minima of unique keys.
//  - ppk_edge_weights_dev : process_weights (PopPUNK/network.py:646-674) of a model edge list: core, accessory or the
//    float32 Euclidean norm of every edge's row of the distance matrix.
#include <cmath>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kNone = 0xffffffffu;   // an empty best slot (ranks are < 2^31)
constexpr int kHops = 16;                 // pointer hops per compression pass
constexpr int kMaxRounds = 32;

// ---- validate ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mst_validate_kernel(const long long *ei, const long long *ej, size_t stride,
                                                                const float *w, size_t m, long long n,
                                                                unsigned long long *bad) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const long long i = ei[k * stride], j = ej[k * stride];
    const bool ok = i >= 0 && i < n && j >= 0 && j < n && i != j && isfinite(w[k]);
    if (!ok) atomicMin(bad, (unsigned long long)k);
  }
}

// ---- rank --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mst_pair_key_kernel(const long long *ei, const long long *ej, size_t stride,
                                                                size_t m, unsigned bits, unsigned long long *keys,
                                                                int *vals) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long i = (unsigned long long)ei[k * stride], j = (unsigned long long)ej[k * stride];
    keys[k] = i < j ? (i << bits) | j : (j << bits) | i;
    vals[k] = (int)k;
  }
}

__global__ void __launch_bounds__(kThreads) mst_weight_key_kernel(const float *w, const int *idx, size_t m,
                                                                  unsigned *keys) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (size_t)gridDim.x * blockDim.x)
    keys[p] = ord_of(w[idx[p]]);      // finite (mst_validate_kernel), -0.0 read as +0.0
}

__global__ void __launch_bounds__(kThreads) mst_ends_kernel(const long long *ei, const long long *ej, size_t stride,
                                                            const int *order, size_t m, int *eu, int *ev) {
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (size_t)gridDim.x * blockDim.x) {
    const size_t k = (size_t)order[r];
    eu[r] = (int)ei[k * stride];
    ev[r] = (int)ej[k * stride];
  }
}

// ---- boruvka -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mst_init_kernel(int *comp, unsigned *best, size_t n) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    comp[v] = (int)v;
    best[v] = kNone;
  }
}

// round > 0 runs only when the round before hooked something.  Ranks ascend along the grid-stride loop, so a plain
// (possibly stale) read of the slot skips most atomics that could not lower it.
__global__ void __launch_bounds__(kThreads) mst_min_kernel(const int *eu, const int *ev, size_t m, const int *comp,
                                                           unsigned *best, const unsigned *hooked, int round) {
  if (round > 0 && hooked[round - 1] == 0) return;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (size_t)gridDim.x * blockDim.x) {
    const int cu = comp[eu[r]], cv = comp[ev[r]];
    if (cu == cv) continue;
    const unsigned rr = (unsigned)r;
    if (best[cu] > rr) atomicMin(&best[cu], rr);
    if (best[cv] > rr) atomicMin(&best[cv], rr);
  }
}

// Every root hooks along its best edge into dst; every other vertex copies its root.  Of a mutual pair (both roots'
// best edge is the same rank) the larger root hooks under the smaller, so the hook graph is a forest.
__global__ void __launch_bounds__(kThreads) mst_hook_kernel(const int *eu, const int *ev, size_t n, const int *comp,
                                                            const unsigned *best, int *dst, unsigned char *chosen,
                                                            unsigned *hooked, int round) {
  if (round > 0 && hooked[round - 1] == 0) return;
  bool any = false;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const int c = comp[v];
    int to = c;
    if (c == (int)v) {
      const unsigned b = best[v];
      if (b != kNone) {
        const int a = comp[eu[b]], z = comp[ev[b]];
        const int other = a == (int)v ? z : a;
        if (!(best[other] == b && (int)v < other)) {
          to = other;
          chosen[b] = 1;
          any = true;
        }
      }
    }
    dst[v] = to;
  }
  if (any) hooked[round] = 1;
}

// One read-only compression pass src -> dst: up to kHops pointer hops per vertex.  A pass that changes nothing
// leaves dst equal to src, so the passes after it may return without touching either.  Pass 0 also empties every
// best slot for the next round.
__global__ void __launch_bounds__(kThreads) mst_jump_kernel(const int *src, int *dst, size_t n, unsigned *best,
                                                            const unsigned *hooked, unsigned *changed, int round,
                                                            int pass) {
  if (hooked[round] == 0) return;
  if (pass > 0 && changed[pass - 1] == 0) return;
  bool any = false;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    if (pass == 0) best[v] = kNone;
    const int x0 = src[v];
    int x = x0;
    for (int h = 0; h < kHops; ++h) {
      const int y = src[x];
      if (y == x) break;
      x = y;
    }
    dst[v] = x;
    any = any || x != x0;
  }
  if (any) changed[pass] = 1;
}

// ---- labels ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mst_fill_kernel(int *a, size_t n, int value) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) a[v] = value;
}

__global__ void __launch_bounds__(kThreads) mst_min_vertex_kernel(const int *comp, size_t n, int *minv) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const int c = comp[v];
    if (minv[c] > (int)v) atomicMin(&minv[c], (int)v);
  }
}

__global__ void __launch_bounds__(kThreads) mst_first_kernel(const int *comp, const int *minv, size_t n, int *first) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    first[v] = minv[comp[v]] == (int)v ? 1 : 0;
}

__global__ void __launch_bounds__(kThreads) mst_label_kernel(const int *comp, const int *minv, const int *rank, size_t n,
                                                             int32_t *labels) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    labels[v] = rank[minv[comp[v]]];
}

// ---- compact -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mst_unrank_kernel(const unsigned char *chosen, const int *order, size_t m,
                                                              unsigned char *flag) {
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (size_t)gridDim.x * blockDim.x)
    flag[order[r]] = chosen[r];
}

// ---- edge weights ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mst_weights_kernel(const float2 *dist, long long n_samples, long long n_ref,
                                                               long long n_qry, long long off, const long long *ei,
                                                               const long long *ej, size_t stride, size_t m, int type,
                                                               float *w, unsigned long long *bad) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const long long i = ei[k * stride], j = ej[k * stride];
    // offsets subtracted before the comparisons: no overflow for ids near the int64 limits
    const long long a = (i < j ? i : j) - off, b = (i < j ? j : i) - off;
    size_t row = 0;
    bool ok;
    if (n_ref == 0) {
      ok = a >= 0 && b < n_samples && a != b;
      if (ok) row = cond_index((size_t)a, (size_t)b, (size_t)n_samples);
    } else {
      ok = a >= 0 && a < n_ref && b >= n_ref && b - n_ref < n_qry;
      if (ok) row = (size_t)(b - n_ref) * (size_t)n_ref + (size_t)a;
    }
    if (!ok) {
      atomicMin(bad, (unsigned long long)k);
      continue;
    }
    const float2 d = dist[row];
    w[k] = type == 0 ? d.x : type == 1 ? d.y : ppk_euclid(d.x, d.y);
  }
}

// process_weights' "euclidean" of rows that are already the edges' own (ppk_dist_pairs_dev's output)
__global__ void __launch_bounds__(kThreads) row_norms_kernel(const float2 *rows, size_t m, float *w) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const float2 d = rows[k];
    w[k] = ppk_euclid(d.x, d.y);
  }
}

int mst_bad_edge(const long long *d_i, const long long *d_j, size_t stride, const float *d_w, size_t k, size_t n) {
  long long i = 0, j = 0;
  float w = 0.0f;
  if (!ppk_read_edge(d_i, d_j, stride, nullptr, k, &i, &j, nullptr))
    return ppk_fail(PPK_ERR_HIP, "cannot read back the bad edge");
  PPK_HIP(hipMemcpy(&w, d_w + k, 4, hipMemcpyDeviceToHost));
  std::string why;
  if (i < 0 || (size_t)i >= n || j < 0 || (size_t)j >= n) why = "vertex id out of range [0, " + std::to_string(n) + ")";
  else if (i == j) why = "self-loop";
  else why = std::isnan(w) ? "NaN weight" : "infinite weight";
  return ppk_fail(PPK_ERR_ARG, "ppk_mst: edge " + std::to_string(k) + " (i=" + std::to_string(i) + ", j=" +
                                   std::to_string(j) + "): " + why);
}

}  // namespace

extern "C" int ppk_mst_dev(const long long *d_i, const long long *d_j, size_t stride, const float *d_w, size_t n_edges,
                           size_t n_vertices, long long *d_tree, unsigned long long *d_n_tree, int32_t *d_labels,
                           void *stream) {
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_mst: n_vertices must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_mst: n_edges must be < 2^31");
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, "ppk_mst: stride must be 1 or 2");
  if (!d_n_tree || (n_edges && (!d_i || !d_j || !d_w || !d_tree)))
    return ppk_fail(PPK_ERR_ARG, "ppk_mst: NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n_edges, n = n_vertices;
  const unsigned bits = (unsigned)(ceil_log2(n) > 0 ? ceil_log2(n) : 1);
  const int rounds = ceil_log2(n) > 0 ? ceil_log2(n) : 1;
  // compression passes per round: 16^passes >= n (the hook forest is no deeper than n), odd so that every round ends
  // with its labels back in comp_a
  int passes = 1;
  while (passes < 8 && ((size_t)1 << (4 * passes)) < n) ++passes;
  if (!(passes & 1)) ++passes;

  size_t sort64 = 0, sort32 = 0, scan_tmp = 0, sel_tmp = 0;
  if (m) {
    PPK_HIP(rocprim::radix_sort_pairs(nullptr, sort64, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                      (int *)nullptr, (int *)nullptr, m, 0u, 2 * bits, s));
    PPK_HIP(rocprim::radix_sort_pairs(nullptr, sort32, (unsigned *)nullptr, (unsigned *)nullptr, (int *)nullptr,
                                      (int *)nullptr, m, 0u, 32u, s));
    PPK_HIP(rocprim::select(nullptr, sel_tmp, rocprim::counting_iterator<long long>(0), (unsigned char *)nullptr,
                            (long long *)nullptr, (unsigned long long *)nullptr, m, s));
  }
  if (n && d_labels)
    PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, (int *)nullptr, (int *)nullptr, 0, n, rocprim::plus<int>(), s));
  size_t tmp = sort64;
  if (sort32 > tmp) tmp = sort32;
  if (scan_tmp > tmp) tmp = scan_tmp;
  if (sel_tmp > tmp) tmp = sel_tmp;

  // scratch: bad | round words | pass words (zeroed up to here) | keys a, b (the 32-bit keys and then the ends reuse
  // them) | values a, b | chosen (by rank) | flags (by index) | comp a, b | best | min vertex | first | rank | temp
  unsigned long long *bad, *ka, *kb;
  unsigned *hooked, *changed, *best;
  int *va, *vb, *ca, *cb, *minv, *first, *rank;
  unsigned char *chosen, *flag;
  char *d_tmp;
  size_t zero_end = 0;
  int rc = ppk_scratch_carve(dev, SLOT_MST, [&](Carve &c) {
    c.take(bad, 1).take(hooked, kMaxRounds).take(changed, (size_t)kMaxRounds * 16);
    zero_end = c.at;
    c.take(ka, m).take(kb, m).take(va, m).take(vb, m).take(chosen, m).take(flag, m);
    c.take(ca, n).take(cb, n).take(best, n).take(minv, n).take(first, n).take(rank, n).take(d_tmp, tmp + 16);
  });
  if (rc != PPK_OK) return rc;
  unsigned *wa = reinterpret_cast<unsigned *>(ka), *wb = wa + m;
  int *eu = reinterpret_cast<int *>(kb), *ev = eu + m;
  const unsigned cap_grid = 4096;

  // -- validate: the one synchronisation
  ppk_prof_stage("validate", s);
  PPK_HIP(hipMemsetAsync(bad, 0, zero_end, s));
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  if (m)
    hipLaunchKernelGGL(mst_validate_kernel, dim3(grid_for(m, kThreads * 8, 2048)), dim3(kThreads), 0, s, d_i, d_j,
                       stride, d_w, m, (long long)n, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 8}}, &h)) != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return mst_bad_edge(d_i, d_j, stride, d_w, (size_t)h[0], n);
  }

  // -- rank: (min, max, index) by a stable sort on the pair, then a stable sort on w
  ppk_prof_stage("rank", s);
  if (m) {
    const unsigned g = grid_for(m, kThreads, cap_grid * 4);
    hipLaunchKernelGGL(mst_pair_key_kernel, dim3(g), dim3(kThreads), 0, s, d_i, d_j, stride, m, bits, ka, va);
    PPK_HIP(hipGetLastError());
    size_t tb = tmp;
    PPK_HIP(rocprim::radix_sort_pairs(d_tmp, tb, ka, kb, va, vb, m, 0u, 2 * bits, s));
    hipLaunchKernelGGL(mst_weight_key_kernel, dim3(g), dim3(kThreads), 0, s, d_w, vb, m, wa);
    PPK_HIP(hipGetLastError());
    tb = tmp;
    PPK_HIP(rocprim::radix_sort_pairs(d_tmp, tb, wa, wb, vb, va, m, 0u, 32u, s));
    hipLaunchKernelGGL(mst_ends_kernel, dim3(g), dim3(kThreads), 0, s, d_i, d_j, stride, va, m, eu, ev);
    PPK_HIP(hipGetLastError());
    PPK_HIP(hipMemsetAsync(chosen, 0, m, s));
  }
  const int *order = va;

  // -- boruvka: labels in ca at the start and end of every round
  ppk_prof_stage("boruvka", s);
  if (n) {
    const unsigned gn = grid_for(n, kThreads, cap_grid);
    hipLaunchKernelGGL(mst_init_kernel, dim3(gn), dim3(kThreads), 0, s, ca, best, n);
    PPK_HIP(hipGetLastError());
    if (m) {
      const unsigned gm = grid_for(m, kThreads * 4, cap_grid);
      for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(mst_min_kernel, dim3(gm), dim3(kThreads), 0, s, eu, ev, m, ca, best, hooked, r);
        hipLaunchKernelGGL(mst_hook_kernel, dim3(gn), dim3(kThreads), 0, s, eu, ev, n, ca, best, cb, chosen, hooked, r);
        for (int p = 0; p < passes; ++p)
          hipLaunchKernelGGL(mst_jump_kernel, dim3(gn), dim3(kThreads), 0, s, (p & 1) ? ca : cb, (p & 1) ? cb : ca,
                             n, best, hooked, changed + 16 * r, r, p);
        PPK_HIP(hipGetLastError());
      }
    }
  }

  // -- labels
  if (d_labels && n) {
    ppk_prof_stage("labels", s);
    const unsigned gn = grid_for(n, kThreads, cap_grid);
    hipLaunchKernelGGL(mst_fill_kernel, dim3(gn), dim3(kThreads), 0, s, minv, n, 0x7fffffff);
    hipLaunchKernelGGL(mst_min_vertex_kernel, dim3(gn), dim3(kThreads), 0, s, ca, n, minv);
    hipLaunchKernelGGL(mst_first_kernel, dim3(gn), dim3(kThreads), 0, s, ca, minv, n, first);
    PPK_HIP(hipGetLastError());
    size_t tb = tmp;
    PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, first, rank, 0, n, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(mst_label_kernel, dim3(gn), dim3(kThreads), 0, s, ca, minv, rank, n, d_labels);
    PPK_HIP(hipGetLastError());
  }

  // -- compact: chosen ranks -> input indices, ascending
  ppk_prof_stage("compact", s);
  if (m) {
    hipLaunchKernelGGL(mst_unrank_kernel, dim3(grid_for(m, kThreads, cap_grid * 4)), dim3(kThreads), 0, s, chosen,
                       order, m, flag);
    PPK_HIP(hipGetLastError());
    size_t tb = tmp;
    PPK_HIP(rocprim::select(d_tmp, tb, rocprim::counting_iterator<long long>(0), flag, d_tree, d_n_tree, m, s));
  } else {
    PPK_HIP(hipMemsetAsync(d_n_tree, 0, 8, s));
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_mst(const long long *i, const long long *j, const float *w, size_t n_edges, size_t n_vertices,
                       int device_id, long long *tree, unsigned long long *n_tree, int32_t *labels) {
  if (!n_tree || (n_edges && (!i || !j || !w || !tree))) return ppk_fail(PPK_ERR_ARG, "ppk_mst: NULL array");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_mst: n_edges must be < 2^31");
  if (n_vertices >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_mst: n_vertices must be < 2^31");
  long long *d_i, *d_j, *d_tree;
  float *d_w;
  int32_t *d_labels;
  unsigned long long *d_n;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_tree, n_edges).take(d_w, n_edges).take(d_labels, n_vertices);
    c.take(d_n, 1);
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_w, w, n_edges * 4, hipMemcpyHostToDevice));
    }
    const int rc =
        ppk_mst_dev(d_i, d_j, 1, d_w, n_edges, n_vertices, d_tree, d_n, labels ? d_labels : nullptr, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(n_tree, d_n, 8, hipMemcpyDeviceToHost));
    if (*n_tree) PPK_HIP(hipMemcpy(tree, d_tree, *n_tree * 8, hipMemcpyDeviceToHost));
    if (labels && n_vertices) PPK_HIP(hipMemcpy(labels, d_labels, n_vertices * 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" int ppk_edge_weights_dev(const float *d_dist, size_t n_rows, const long long *d_i, const long long *d_j,
                                    size_t stride, size_t n_edges, size_t n_ref, long long int_offset, int weights_type,
                                    float *d_w, void *stream) {
  if (weights_type < 0 || weights_type > 2)
    return ppk_fail(PPK_ERR_ARG, "ppk_edge_weights: weights_type must be 0 (core), 1 (accessory) or 2 (euclidean)");
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, "ppk_edge_weights: stride must be 1 or 2");
  if (n_edges && (!d_dist || !d_i || !d_j || !d_w)) return ppk_fail(PPK_ERR_ARG, "ppk_edge_weights: NULL array");
  if (n_rows >= ((size_t)1 << 62)) return ppk_fail(PPK_ERR_ARG, "ppk_edge_weights: n_rows too large");
  size_t n_samples = 0, n_qry = 0;
  if (n_ref == 0) {
    if (int rc = ppk_condensed_samples(n_rows, &n_samples, "ppk_edge_weights: ", "self matrix")) return rc;
  } else {
    if (n_rows % n_ref) return ppk_fail(PPK_ERR_ARG, "ppk_edge_weights: row count is not a multiple of n_ref");
    n_qry = n_rows / n_ref;
  }
  if (!n_edges) return PPK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  unsigned long long *bad;
  int rc = ppk_scratch_carve(dev, SLOT_MST, [&](Carve &c) { c.take(bad, 1); });
  if (rc != PPK_OK) return rc;
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  hipLaunchKernelGGL(mst_weights_kernel, dim3(grid_for(n_edges, kThreads * 4, 4096)), dim3(kThreads), 0, s,
                     reinterpret_cast<const float2 *>(d_dist), (long long)n_samples, (long long)n_ref, (long long)n_qry,
                     int_offset, d_i, d_j, stride, n_edges, weights_type, d_w, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 8}}, &h)) != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    long long i = 0, j = 0;
    if (!ppk_read_edge(d_i, d_j, stride, nullptr, (size_t)h[0], &i, &j, nullptr))
      return ppk_fail(PPK_ERR_HIP, "cannot read back the bad edge");
    return ppk_fail(PPK_ERR_ARG, "ppk_edge_weights: edge " + std::to_string(h[0]) + " (i=" + std::to_string(i) +
                                     ", j=" + std::to_string(j) + ") has no row in the distance matrix");
  }
  return PPK_OK;
}

extern "C" int ppk_row_norms_dev(const float *d_rows, size_t n_rows, float *d_w, void *stream) {
  if (n_rows && (!d_rows || !d_w)) return ppk_fail(PPK_ERR_ARG, "ppk_row_norms: NULL array");
  if (!n_rows) return PPK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(row_norms_kernel, dim3(grid_for(n_rows, kThreads * 4, 4096)), dim3(kThreads), 0, s,
                     reinterpret_cast<const float2 *>(d_rows), n_rows, d_w);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

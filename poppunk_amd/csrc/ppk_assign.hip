// Which components of the loaded network is every query linked to.
//
//  - ppk_query_links_dev : per query its number of query-reference edges, the exact number of distinct component
//    labels among the references at their other ends, and the smallest max_links of those labels.  It stands in for
//    the Python set that qcQueryAssignments walks per query over the [n_qry * n_ref] assignment (PopPUNK/qc.py:372-417)
//    and, under `serial`, for the graph copy + label_components per query of assign_query_hdf5 (PopPUNK/assign.py:
//    696-722): the reference network enters only through label[r].
//    Stages (ppk_prof_stages names):
//      validate   every id and self-loop, every label; and whether the stream is ORDERED: the key of an edge is its
//                 query for a query-reference edge and n_qry for an edge that is skipped (both ends on one side), and
//                 the keys never decrease.  Every producer emits row order, so this is the usual case.  The call's
//                 synchronisation reads the first bad edge, the first bad label and that flag.
//    ordered:
//      segments   start[q] = the first edge of key q (each edge fills the starts between its predecessor's key and its
//                 own, as net_segments_kernel does)
//      links      one wave per query: 64 edges at a time, label[r] per lane; the leader's label (lowest pending lane)
//                 is broadcast, inserted once and retired on every lane that holds it (ps_wave_add's ballot-on-leader,
//                 ppk_clusters.hip), twice, and what is left goes lane by lane; all into an LDS set of
//                 PPK_ASSIGN_SET_CAP entries (open addressing, compare-and-swap).  A set that fills up puts the query
//                 on the overflow list with a reserved range of the key buffer.  Otherwise every entry's rank is a
//                 count of the smaller entries and the first max_links are written in place.
//      overflow   (only when the list is not empty: a second, 16-byte read-back says so) the listed queries' (query,
//                 label) keys, then the sort route below on those keys alone
//    not ordered:
//      keys       (query, label) of every query-reference edge, the degree by integer atomics; then the sort route
//    sort route:  rocPRIM radix sort of the keys, a flag at the first of every run of equal keys, rocPRIM exclusive scan
//                 of the flags = the index of a distinct key; minus that index at the query's first key = the label's
//                 rank within the query.
//    Everything is integer; the links of a query are written by one wave or derived from sorted positions, so the bits
//    do not depend on the order the atomics land in.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSetCap = PPK_ASSIGN_SET_CAP;
static_assert(kSetCap == 128, "the set's hash takes 7 bits and a lane holds two entries");
constexpr unsigned long long kNone = ~0ull;
enum { C_BAD_EDGE, C_BAD_LABEL, C_UNORDERED, C_N_OVF, C_OVF_EDGES, C_LEN };
const std::string kWho = "ppk_query_links";

// the query of a valid query-reference edge; n_qry for every other edge
__device__ __forceinline__ unsigned al_key(long long i, long long j, long long n_ref, long long n, unsigned n_qry,
                                           bool *valid = nullptr) {
  const bool ok = i >= 0 && i < n && j >= 0 && j < n && i != j;
  if (valid) *valid = ok;
  if (!ok || (i >= n_ref) == (j >= n_ref)) return n_qry;
  return (unsigned)((i >= n_ref ? i : j) - n_ref);
}

__global__ void __launch_bounds__(kThreads) al_validate_kernel(const long long *ei, const long long *ej, size_t stride,
                                                               size_t m, long long n_ref, unsigned n_qry,
                                                               unsigned long long *ctr) {
  const long long n = n_ref + n_qry;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    bool ok;
    const unsigned key = al_key(ei[k * stride], ej[k * stride], n_ref, n, n_qry, &ok);
    if (!ok) atomicMin(&ctr[C_BAD_EDGE], (unsigned long long)k);
    if (k && al_key(ei[(k - 1) * stride], ej[(k - 1) * stride], n_ref, n, n_qry) > key) ctr[C_UNORDERED] = 1;
  }
}
__global__ void __launch_bounds__(kThreads) al_labels_kernel(const int32_t *label, size_t n_ref,
                                                             unsigned long long *ctr) {
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_ref; r += (size_t)gridDim.x * blockDim.x) {
    const long long l = label[r];
    if (l < 0 || l >= (long long)n_ref) atomicMin(&ctr[C_BAD_LABEL], (unsigned long long)r);
  }
}

// ---- ordered: segment starts (start has n_qry + 2 entries: the skipped edges are segment n_qry) --------------------
__global__ void __launch_bounds__(kThreads) al_segments_kernel(const long long *ei, const long long *ej, size_t stride,
                                                               size_t m, long long n_ref, unsigned n_qry,
                                                               unsigned *start) {
  const long long n = n_ref + n_qry;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned key = al_key(ei[p * stride], ej[p * stride], n_ref, n, n_qry);
    const unsigned first = p ? al_key(ei[(p - 1) * stride], ej[(p - 1) * stride], n_ref, n, n_qry) + 1 : 0;
    for (unsigned x = first; x <= key; ++x) start[x] = (unsigned)p;
    if (p == m - 1)
      for (unsigned x = key + 1; x <= n_qry + 1; ++x) start[x] = (unsigned)m;
  }
}

// ---- ordered: one wave (= one workgroup) per query ------------------------------------------------------------------
__device__ __forceinline__ void al_insert(int *set, int *full, int label) {
  const unsigned h = ((unsigned)label * 0x9E3779B1u) >> 25;
  for (int t = 0; t < kSetCap; ++t) {
    const int old = atomicCAS(&set[(h + t) & (kSetCap - 1)], -1, label);
    if (old == -1 || old == label) return;
  }
  *full = 1;
}

__global__ void __launch_bounds__(64) al_links_kernel(const long long *ei, const long long *ej, size_t stride,
                                                      const int32_t *label, long long n_ref, unsigned n_qry,
                                                      const unsigned *start, int max_links, int32_t *degree,
                                                      int32_t *n_links, int32_t *links, unsigned long long *ctr,
                                                      unsigned *ovf_q, unsigned *ovf_off) {
  __shared__ int set[kSetCap];
  __shared__ int full;
  const int lane = threadIdx.x;
  for (unsigned q = blockIdx.x; q < n_qry; q += gridDim.x) {
    set[lane] = -1;
    set[lane + 64] = -1;
    if (lane == 0) full = 0;
    __syncthreads();
    const unsigned a = start[q], b = start[q + 1];
    for (unsigned base = a; base < b; base += 64) {          // (wave-uniform)
      const unsigned p = base + lane;
      int key = -1;
      if (p < b) {
        const long long i = ei[(size_t)p * stride], j = ej[(size_t)p * stride];
        key = label[i < n_ref ? i : j];
      }
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const unsigned long long pend = __ballot(key >= 0);
        if (!pend) break;                                    // (wave-uniform)
        const int leader = __ffsll((long long)pend) - 1;
        const int k0 = __shfl(key, leader);
        if (lane == leader) al_insert(set, &full, k0);
        if (key == k0) key = -1;
      }
      if (key >= 0) al_insert(set, &full, key);
    }
    __syncthreads();
    if (lane == 0) degree[q] = (int32_t)(b - a);
    if (full) {
      if (lane == 0) {
        const unsigned slot = (unsigned)atomicAdd(&ctr[C_N_OVF], 1ull);
        ovf_q[slot] = q;
        ovf_off[slot] = (unsigned)atomicAdd(&ctr[C_OVF_EDGES], (unsigned long long)(b - a));
      }
    } else {
      const int v0 = set[lane], v1 = set[lane + 64];
      int r0 = 0, r1 = 0, total = 0;
      for (int t = 0; t < kSetCap; ++t) {
        const int x = set[t];                                // (broadcast read)
        if (x < 0) continue;
        ++total;
        r0 += x < v0;
        r1 += x < v1;
      }
      if (v0 >= 0 && r0 < max_links) links[(size_t)q * max_links + r0] = v0;
      if (v1 >= 0 && r1 < max_links) links[(size_t)q * max_links + r1] = v1;
      if (lane == 0) n_links[q] = total;
    }
    __syncthreads();
  }
}

// the keys of the overflow list's queries, each in its reserved range
__global__ void __launch_bounds__(64) al_overflow_keys_kernel(const long long *ei, const long long *ej, size_t stride,
                                                              const int32_t *label, long long n_ref,
                                                              const unsigned *start, const unsigned *ovf_q,
                                                              const unsigned *ovf_off, unsigned n_ovf,
                                                              unsigned long long *keys) {
  for (unsigned slot = blockIdx.x; slot < n_ovf; slot += gridDim.x) {
    const unsigned q = ovf_q[slot], a = start[q], len = start[q + 1] - a;
    unsigned long long *out = keys + ovf_off[slot];
    for (unsigned t = threadIdx.x; t < len; t += blockDim.x) {
      const long long i = ei[(size_t)(a + t) * stride], j = ej[(size_t)(a + t) * stride];
      out[t] = (unsigned long long)q << 32 | (unsigned)label[i < n_ref ? i : j];
    }
  }
}

// ---- not ordered: a key per edge, kNone for a skipped one; the degrees ------------------------------------------------
__global__ void __launch_bounds__(kThreads) al_keys_kernel(const long long *ei, const long long *ej, size_t stride,
                                                           size_t m, const int32_t *label, long long n_ref,
                                                           unsigned n_qry, unsigned long long *keys, int32_t *degree) {
  const long long n = n_ref + n_qry;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const long long i = ei[k * stride], j = ej[k * stride];
    const unsigned q = al_key(i, j, n_ref, n, n_qry);
    if (q == n_qry) {
      keys[k] = kNone;
    } else {
      keys[k] = (unsigned long long)q << 32 | (unsigned)label[i < n_ref ? i : j];
      atomicAdd(&degree[q], 1);
    }
  }
}

// ---- sort route: distinct keys and their ranks ------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) al_flags_kernel(const unsigned long long *sorted, size_t cnt,
                                                            unsigned *flag) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < cnt; p += (size_t)gridDim.x * blockDim.x)
    flag[p] = sorted[p] != kNone && (p == 0 || sorted[p - 1] != sorted[p]);
}
// qfirst[q] = the index, among the distinct keys, of the query's first key
__global__ void __launch_bounds__(kThreads) al_first_kernel(const unsigned long long *sorted, size_t cnt,
                                                            const unsigned *idx, unsigned *qfirst) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < cnt; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = sorted[p];
    if (key != kNone && (p == 0 || (sorted[p - 1] >> 32) != (key >> 32))) qfirst[key >> 32] = idx[p];
  }
}
__global__ void __launch_bounds__(kThreads) al_emit_kernel(const unsigned long long *sorted, size_t cnt,
                                                           const unsigned *flag, const unsigned *idx,
                                                           const unsigned *qfirst, int max_links, int32_t *n_links,
                                                           int32_t *links) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < cnt; p += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long key = sorted[p];
    if (key == kNone) continue;
    const size_t q = key >> 32;
    const unsigned rank = idx[p] - qfirst[q];                // (of this key if it opens a run, else of the next run)
    if (flag[p] && rank < (unsigned)max_links) links[q * max_links + rank] = (int32_t)(key & 0xffffffffu);
    if (p + 1 == cnt || sorted[p + 1] == kNone || (sorted[p + 1] >> 32) != q) n_links[q] = (int32_t)(rank + flag[p]);
  }
}

int links_from_keys(int dev, hipStream_t s, unsigned long long *keys, unsigned long long *sorted, unsigned *flag,
                    unsigned *idx, char *d_tmp, size_t tmp, size_t cnt, unsigned end_bit, unsigned *qfirst,
                    int max_links, int32_t *d_n_links, int32_t *d_links) {
  size_t tb = tmp;
  PPK_HIP(rocprim::radix_sort_keys(d_tmp, tb, keys, sorted, cnt, 0u, end_bit, s));
  const dim3 g(grid_for(cnt, kThreads * 4, 4096));
  hipLaunchKernelGGL(al_flags_kernel, g, dim3(kThreads), 0, s, sorted, cnt, flag);
  tb = tmp;
  PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, flag, idx, 0u, cnt, rocprim::plus<unsigned>(), s));
  hipLaunchKernelGGL(al_first_kernel, g, dim3(kThreads), 0, s, sorted, cnt, idx, qfirst);
  hipLaunchKernelGGL(al_emit_kernel, g, dim3(kThreads), 0, s, sorted, cnt, flag, idx, qfirst, max_links, d_n_links,
                     d_links);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_query_links_dev(const long long *d_i, const long long *d_j, size_t stride, size_t n_edges,
                                   const int32_t *d_ref_label, size_t n_ref, size_t n_qry, int max_links,
                                   int32_t *d_degree, int32_t *d_n_links, int32_t *d_links, void *stream) {
  const std::string &who = kWho;
  if (max_links < 1 || max_links > 64) return ppk_fail(PPK_ERR_ARG, who + ": max_links must be 1 .. 64");
  if (n_ref >= ((size_t)1 << 31) || n_qry >= ((size_t)1 << 31) || n_ref + n_qry >= ((size_t)1 << 31))
    return ppk_fail(PPK_ERR_ARG, who + ": n_ref + n_qry must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_edges must be < 2^31");
  if (stride != 1 && stride != 2) return ppk_fail(PPK_ERR_ARG, who + ": stride must be 1 or 2");
  if ((n_edges && (!d_i || !d_j)) || (n_ref && !d_ref_label) || (n_qry && (!d_degree || !d_n_links || !d_links)))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n_edges, nq = n_qry;
  const size_t n = n_ref + n_qry;

  unsigned long long *ctr;
  unsigned *start, *ovf_q, *ovf_off, *qfirst;
  int rc = ppk_scratch_carve(dev, SLOT_ASSIGN, [&](Carve &c) {
    c.take(ctr, C_LEN).take(start, nq + 2).take(ovf_q, nq).take(ovf_off, nq).take(qfirst, nq);
  });
  if (rc != PPK_OK) return rc;

  // -- validate: the first offender and whether the stream is ordered
  ppk_prof_stage("validate", s);
  PPK_HIP(hipMemsetAsync(ctr, 0xff, 16, s));
  PPK_HIP(hipMemsetAsync(ctr + C_UNORDERED, 0, (C_LEN - C_UNORDERED) * 8, s));
  if (n_ref)
    hipLaunchKernelGGL(al_labels_kernel, dim3(grid_for(n_ref, kThreads * 4, 2048)), dim3(kThreads), 0, s, d_ref_label,
                       n_ref, ctr);
  if (m)
    hipLaunchKernelGGL(al_validate_kernel, dim3(grid_for(m, kThreads * 8, 2048)), dim3(kThreads), 0, s, d_i, d_j, stride,
                       m, (long long)n_ref, (unsigned)nq, ctr);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{ctr, 24}}, &h)) != PPK_OK) return rc;
  if (h[C_BAD_LABEL] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    int32_t l = 0;
    PPK_HIP(hipMemcpy(&l, d_ref_label + h[C_BAD_LABEL], 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": reference " + std::to_string(h[C_BAD_LABEL]) + ": label " + std::to_string(l) +
                                     " outside [0, " + std::to_string(n_ref) + ")");
  }
  if (h[C_BAD_EDGE] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    const size_t k = (size_t)h[C_BAD_EDGE];
    long long i = 0, j = 0;
    if (!ppk_read_edge(d_i, d_j, stride, nullptr, k, &i, &j, nullptr))
      return ppk_fail(PPK_ERR_HIP, who + ": cannot read back the bad edge");
    const bool range = i < 0 || (size_t)i >= n || j < 0 || (size_t)j >= n;
    return ppk_fail(PPK_ERR_ARG, who + ": edge " + std::to_string(k) + " (i=" + std::to_string(i) + ", j=" +
                                     std::to_string(j) + "): " +
                                     (range ? "vertex id out of range [0, " + std::to_string(n) + ")" : "self-loop"));
  }
  const bool ordered = h[C_UNORDERED] == 0;
  if (!nq) {
    ppk_prof_stage(nullptr, s);
    return PPK_OK;
  }
  PPK_HIP(hipMemsetAsync(d_degree, 0, nq * 4, s));
  PPK_HIP(hipMemsetAsync(d_n_links, 0, nq * 4, s));
  PPK_HIP(hipMemsetAsync(d_links, 0xff, nq * (size_t)max_links * 4, s));
  if (!m) {
    ppk_prof_stage(nullptr, s);
    return PPK_OK;
  }

  size_t cnt = m;                        // keys on the sort route
  if (ordered) {
    ppk_prof_stage("segments", s);
    hipLaunchKernelGGL(al_segments_kernel, dim3(grid_for(m, kThreads, 8192)), dim3(kThreads), 0, s, d_i, d_j, stride, m,
                       (long long)n_ref, (unsigned)nq, start);
    ppk_prof_stage("links", s);
    hipLaunchKernelGGL(al_links_kernel, dim3(grid_for(nq, 1, 1u << 16)), dim3(64), 0, s, d_i, d_j, stride, d_ref_label,
                       (long long)n_ref, (unsigned)nq, start, max_links, d_degree, d_n_links, d_links, ctr, ovf_q,
                       ovf_off);
    PPK_HIP(hipGetLastError());
    if ((rc = ppk_read_back(dev, s, {{ctr + C_N_OVF, 16}}, &h)) != PPK_OK) return rc;
    if (!h[0]) {
      ppk_prof_stage(nullptr, s);
      return PPK_OK;
    }
    cnt = (size_t)h[1];
  }
  const unsigned n_ovf = ordered ? (unsigned)h[0] : 0;

  // -- the sort route: the overflow list's keys, or every edge's
  ppk_prof_stage(ordered ? "overflow" : "keys", s);
  const unsigned end_bit = 32 + (unsigned)ceil_log2(nq) + 1;     // kNone sorts after every query's keys
  size_t sort_tmp = 0, scan_tmp = 0;
  PPK_HIP(rocprim::radix_sort_keys(nullptr, sort_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr, cnt,
                                   0u, end_bit, s));
  PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, (unsigned *)nullptr, (unsigned *)nullptr, 0u, cnt,
                                  rocprim::plus<unsigned>(), s));
  const size_t tmp = sort_tmp > scan_tmp ? sort_tmp : scan_tmp;
  unsigned long long *keys, *sorted;
  unsigned *flag, *idx;
  char *d_tmp;
  rc = ppk_scratch_carve(dev, SLOT_ASSIGN_SORT, [&](Carve &c) {
    c.take(keys, cnt).take(sorted, cnt).take(flag, cnt).take(idx, cnt).take(d_tmp, tmp + 16);
  });
  if (rc != PPK_OK) return rc;
  if (ordered)
    hipLaunchKernelGGL(al_overflow_keys_kernel, dim3(grid_for(n_ovf, 1, 1u << 16)), dim3(64), 0, s, d_i, d_j, stride,
                       d_ref_label, (long long)n_ref, start, ovf_q, ovf_off, n_ovf, keys);
  else
    hipLaunchKernelGGL(al_keys_kernel, dim3(grid_for(m, kThreads * 4, 4096)), dim3(kThreads), 0, s, d_i, d_j, stride, m,
                       d_ref_label, (long long)n_ref, (unsigned)nq, keys, d_degree);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage("sort", s);
  rc = links_from_keys(dev, s, keys, sorted, flag, idx, d_tmp, tmp, cnt, end_bit, qfirst, max_links, d_n_links, d_links);
  ppk_prof_stage(nullptr, s);
  return rc;
}

extern "C" int ppk_query_links(const long long *i, const long long *j, size_t n_edges, const int32_t *ref_label,
                               size_t n_ref, size_t n_qry, int max_links, int device_id, int32_t *degree,
                               int32_t *n_links, int32_t *links) {
  const std::string &who = kWho;
  if (max_links < 1 || max_links > 64) return ppk_fail(PPK_ERR_ARG, who + ": max_links must be 1 .. 64");
  if (n_ref >= ((size_t)1 << 31) || n_qry >= ((size_t)1 << 31) || n_ref + n_qry >= ((size_t)1 << 31))
    return ppk_fail(PPK_ERR_ARG, who + ": n_ref + n_qry must be < 2^31");
  if (n_edges >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_edges must be < 2^31");
  if ((n_edges && (!i || !j)) || (n_ref && !ref_label) || (n_qry && (!degree || !n_links || !links)))
    return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  long long *d_i, *d_j;
  int32_t *d_label, *d_degree, *d_n_links, *d_links;
  const size_t ml = (size_t)max_links;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, n_edges).take(d_j, n_edges).take(d_label, n_ref);
    c.take(d_degree, n_qry).take(d_n_links, n_qry).take(d_links, n_qry * ml);
  }, [&]() -> int {
    if (n_edges) {
      PPK_HIP(hipMemcpy(d_i, i, n_edges * 8, hipMemcpyHostToDevice));
      PPK_HIP(hipMemcpy(d_j, j, n_edges * 8, hipMemcpyHostToDevice));
    }
    if (n_ref) PPK_HIP(hipMemcpy(d_label, ref_label, n_ref * 4, hipMemcpyHostToDevice));
    const int rc = ppk_query_links_dev(d_i, d_j, 1, n_edges, d_label, n_ref, n_qry, max_links, d_degree, d_n_links,
                                       d_links, nullptr);
    if (rc != PPK_OK) return rc;
    if (n_qry) {
      PPK_HIP(hipMemcpy(degree, d_degree, n_qry * 4, hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(n_links, d_n_links, n_qry * 4, hipMemcpyDeviceToHost));
      PPK_HIP(hipMemcpy(links, d_links, n_qry * ml * 4, hipMemcpyDeviceToHost));
    }
    return PPK_OK;
  });
}

// Neighbour-joining trees on the device.
//
//  - ppk_nj_dev : exact neighbour joining of a core-distance matrix with the join and tie rule of Biopython's
//    DistanceTreeConstructor.nj (the default branch of generate_nj_tree, PopPUNK/trees.py:157-197).  Working values
//    are float64, every expression un-fused and in Biopython's order of operations; the row sums follow this
//    library's own O(1) rule (ppk.h).  Stages (ppk_prof_stages names):
//      load        the strictly lower triangle into a float64 working triangle, checked finite; the call's ONE
//                  synchronisation reads the first bad entry
//      rowsum      every row's sum in ascending column order
//      scan        one launch per join: each workgroup streams its share of the active triangle, computes Q and
//                  writes its best (Q, triangle index) to its own slot
//      update      one launch per join: every workgroup reduces those slots in a fixed order (the minimum of a total
//                  order, so no atomics and no dependence on arrival order), then writes the joined row, the row
//                  sums and, from workgroup 0, the join record
//      compact     when an eighth of the slots have gone: the active nodes into a dense triangle (ping-pong buffers)
//      tail        the last kTailR joins and the final edge in one single-workgroup launch
//    Kernel boundaries are the only hand-offs between workgroups; the only atomic is the load's integer minimum.
#include <cmath>
#include <cstring>
#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTailThreads = 1024;
constexpr unsigned kMaxParts = 2048;     // scan workgroups (and best slots) at most
constexpr size_t kPerPart = 2048;        // triangle entries a scan workgroup takes at least
constexpr long long kTailR = 256;        // active nodes from which one workgroup finishes the tree
constexpr long long kPoll = 256;         // joins between two interrupt checks

struct Best {
  double q;
  unsigned long long e;
};

// (q, e) lexicographic: the smaller Q, then the smaller triangle index (the smaller a, then the smaller b).  -0.0 and
// +0.0 compare equal.
__device__ __forceinline__ bool better(double q, unsigned long long e, double bq, unsigned long long be) {
  return q < bq || (q == bq && e < be);
}

// The minimum of every thread's (q, e) over the block, returned to every thread (blockDim.x a power of two <= 1024).
__device__ void block_min(double &q, unsigned long long &e) {
  __shared__ double sq[kTailThreads];
  __shared__ unsigned long long se[kTailThreads];
  const unsigned tid = threadIdx.x;
  sq[tid] = q;
  se[tid] = e;
  __syncthreads();
  for (unsigned h = blockDim.x / 2; h > 0; h >>= 1) {
    if (tid < h && better(sq[tid + h], se[tid + h], sq[tid], se[tid])) {
      sq[tid] = sq[tid + h];
      se[tid] = se[tid + h];
    }
    __syncthreads();
  }
  q = sq[0];
  e = se[0];
  __syncthreads();
}

// The best (Q, e) of triangle entries [e0, e1) of active pairs, per thread: entries ascend along a thread's loop, so
// a strict < keeps the first of equal Q.
__device__ void scan_range(const double *__restrict__ W, const unsigned char *__restrict__ alive,
                           const double *__restrict__ nd, size_t e0, size_t e1, double &bq, unsigned long long &be) {
  const size_t step = blockDim.x;
  size_t x = e0 + threadIdx.x;
  if (x >= e1) return;
  size_t a = row_of(x), b = x - tri(a);
  for (; x < e1; x += step) {
    if (alive[a] && alive[b]) {
      const double q = (W[x] - nd[a]) - nd[b];
      if (q < bq) {
        bq = q;
        be = x;
      }
    }
    b += step;
    while (b >= a) {
      b -= a;
      ++a;
    }
  }
}

__global__ void __launch_bounds__(kThreads) nj_scan_kernel(const double *__restrict__ W,
                                                           const unsigned char *__restrict__ alive,
                                                           const double *__restrict__ nd, size_t m, Best *part) {
  const size_t T = tri(m), chunk = (T + gridDim.x - 1) / gridDim.x;
  const size_t e0 = (size_t)blockIdx.x * chunk, e1 = e0 + chunk < T ? e0 + chunk : T;
  double q = INFINITY;
  unsigned long long e = ~0ull;
  if (e0 < e1) scan_range(W, alive, nd, e0, e1, q, e);
  block_min(q, e);
  if (threadIdx.x == 0) part[blockIdx.x] = Best{q, e};
}

// Join the pair at triangle entry e (a > b) while r nodes are active: row b becomes the new node, slot a goes.  The
// grid strides over the other slots k; block 0's thread 0 writes the record and slot b's own values.
__device__ void join_pair(double *W, unsigned char *alive, double *S, double *nd, long long *ids, size_t m,
                          unsigned long long e, long long r, long long t, long long n, long long *join, double *len) {
  if (e >= tri(m)) return;   // no active pair (not reached for r > 2 and finite input)
  const size_t a = row_of((size_t)e), b = (size_t)e - tri(a);
  const double dab = W[e];
  const long long nr = r - 1;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    if (k == a || k == b || !alive[k]) continue;
    const size_t ib = tidx(b, k);
    const double dak = W[tidx(a, k)], dbk = W[ib];
    const double dn = ((dak + dbk) - dab) / 2.0;
    W[ib] = dn;
    const double s = ((S[k] - dak) - dbk) + dn;
    S[k] = s;
    if (nr > 2) nd[k] = s / (double)(nr - 2);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double la = ((dab + nd[a]) - nd[b]) / 2.0;
    join[2 * t] = ids[a];
    join[2 * t + 1] = ids[b];
    len[2 * t] = la;
    len[2 * t + 1] = dab - la;
    const double sb = ((S[a] + S[b]) - (double)r * dab) / 2.0;
    S[b] = sb;
    if (nr > 2) nd[b] = sb / (double)(nr - 2);
    ids[b] = n + t;
    alive[a] = 0;
  }
}

__global__ void __launch_bounds__(kThreads) nj_update_kernel(double *W, unsigned char *alive, double *S, double *nd,
                                                             long long *ids, const Best *part, unsigned n_parts,
                                                             size_t m, long long r, long long t, long long n,
                                                             long long *join, double *len) {
  double q = INFINITY;
  unsigned long long e = ~0ull;
  for (unsigned i = threadIdx.x; i < n_parts; i += blockDim.x)
    if (better(part[i].q, part[i].e, q, e)) {
      q = part[i].q;
      e = part[i].e;
    }
  block_min(q, e);
  join_pair(W, alive, S, nd, ids, m, e, r, t, n, join, len);
}

// The joins from r active nodes down to 2, then the final edge, in one workgroup.  Global writes of one step are
// read by other threads of the same workgroup after a barrier.
__global__ void __launch_bounds__(kTailThreads) nj_tail_kernel(double *W, unsigned char *alive, double *S, double *nd,
                                                               long long *ids, size_t m, long long r, long long t,
                                                               long long n, long long *join, double *len) {
  for (; r > 2; --r, ++t) {
    double q = INFINITY;
    unsigned long long e = ~0ull;
    scan_range(W, alive, nd, 0, tri(m), q, e);
    block_min(q, e);
    join_pair(W, alive, S, nd, ids, m, e, r, t, n, join, len);
    __syncthreads();
  }
  if (threadIdx.x == 0 && r == 2) {
    size_t p0 = 0;
    while (p0 + 1 < m && !alive[p0]) ++p0;
    size_t p1 = p0 + 1;
    while (p1 < m && !alive[p1]) ++p1;
    if (p1 >= m) return;
    const double d = W[tri(p1) + p0];
    join[2 * (n - 2)] = ids[p1];
    join[2 * (n - 2) + 1] = ids[p0];
    len[2 * (n - 2)] = d;
    len[2 * (n - 2) + 1] = d;
  }
}

// ---- load / rowsum -------------------------------------------------------------------------------------------------
// One block per row a (grid-stride): W[tri(a) + b] = D[a, b] for b < a, from the square (row a) or the long form
// (condensed entry of (b, a)).  The first non-finite entry's triangle index is kept by an integer minimum.
__global__ void __launch_bounds__(kThreads) nj_load_kernel(const float *src, int kind, size_t stride, size_t col,
                                                           size_t n, double *W, unsigned long long *bad) {
  for (size_t a = 1 + blockIdx.x; a < n; a += gridDim.x) {
    for (size_t b = threadIdx.x; b < a; b += blockDim.x) {
      const float v = kind == PPK_NJ_SQUARE ? src[a * n + b]
                                            : src[(b * n - b * (b + 1) / 2 + (a - b - 1)) * stride + col];
      if (!isfinite(v)) atomicMin(bad, (unsigned long long)(tri(a) + b));
      W[tri(a) + b] = (double)v;
    }
  }
}

// S[k] = D[k, 0] + D[k, 1] + ... + D[k, n-1] from +0.0, in ascending column order, the diagonal skipped.
__global__ void __launch_bounds__(kThreads) nj_rowsum_kernel(const double *__restrict__ W, size_t n, double *S,
                                                             double *nd, long long *ids, unsigned char *alive) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  constexpr int kU = 8;
  double s = 0.0;
  for (size_t j0 = 0; j0 < n; j0 += kU) {
    double v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const size_t j = j0 + u;
      v[u] = (j < n && j != k) ? W[tidx(k, j)] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (j0 + u < n && j0 + u != k) s += v[u];
  }
  S[k] = s;
  nd[k] = n > 2 ? s / (double)(n - 2) : 0.0;
  ids[k] = (long long)k;
  alive[k] = 1;
}

// ---- compact -------------------------------------------------------------------------------------------------------
// One block: the active slots of [0, m) in order -> new slots 0 .. r-1 (old_of[new] = old), their S, nd and ids.
__global__ void __launch_bounds__(kTailThreads) nj_compact_map_kernel(const unsigned char *alive, const double *S,
                                                                      const double *nd, const long long *ids, size_t m,
                                                                      unsigned *old_of, double *S2, double *nd2,
                                                                      long long *ids2, unsigned char *alive2) {
  __shared__ unsigned sc[kTailThreads];
  const unsigned tid = threadIdx.x;
  size_t base_new = 0;
  for (size_t base = 0; base < m; base += blockDim.x) {
    const size_t k = base + tid;
    const unsigned f = (k < m && alive[k]) ? 1u : 0u;
    sc[tid] = f;
    __syncthreads();
    for (unsigned h = 1; h < blockDim.x; h <<= 1) {   // inclusive Hillis-Steele scan
      const unsigned v = tid >= h ? sc[tid - h] : 0u;
      __syncthreads();
      sc[tid] += v;
      __syncthreads();
    }
    if (f) {
      const size_t p = base_new + sc[tid] - 1;
      old_of[p] = (unsigned)k;
      S2[p] = S[k];
      nd2[p] = nd[k];
      ids2[p] = ids[k];
      alive2[p] = 1;
    }
    base_new += sc[blockDim.x - 1];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads) nj_compact_copy_kernel(const double *__restrict__ W,
                                                                   const unsigned *__restrict__ old_of, size_t r,
                                                                   double *__restrict__ W2) {
  for (size_t a = 1 + blockIdx.x; a < r; a += gridDim.x) {
    const size_t oa = tri(old_of[a]);
    for (size_t b = threadIdx.x; b < a; b += blockDim.x) W2[tri(a) + b] = W[oa + old_of[b]];
  }
}

unsigned scan_parts(size_t m) {
  const size_t g = (tri(m) + kPerPart - 1) / kPerPart;
  return (unsigned)(g < 1 ? 1 : g > kMaxParts ? kMaxParts : g);
}

// the host's schedule: compaction before the join at r active of a triangle of m slots
bool compact_due(long long r, long long m) { return 8 * (m - r) >= m; }

// the largest triangle a compaction writes: the first one's (all later ones are smaller)
size_t first_compaction(long long n) {
  long long m = n;
  for (long long r = n; r > kTailR; --r)
    if (compact_due(r, m)) return (size_t)r;
  return (size_t)(m > kTailR ? kTailR : m);
}

int nj_bad_entry(const float *src, int kind, size_t stride, size_t col, size_t n, size_t e) {
  const size_t a = row_of(e), b = e - tri(a);
  const size_t off = kind == PPK_NJ_SQUARE ? a * n + b : (b * n - b * (b + 1) / 2 + (a - b - 1)) * stride + col;
  float v = 0.0f;
  PPK_HIP(hipMemcpy(&v, src + off, 4, hipMemcpyDeviceToHost));
  return ppk_fail(PPK_ERR_ARG, "ppk_nj: entry (" + std::to_string(a) + ", " + std::to_string(b) + ") is " +
                                   (std::isnan(v) ? "NaN" : "infinite"));
}

}  // namespace

extern "C" int ppk_nj_dev(const float *d_src, int src_kind, size_t stride, size_t col, size_t n, long long *d_join,
                          double *d_len, void *stream) {
  if (n == 0) return ppk_fail(PPK_ERR_ARG, "ppk_nj: n must be at least 1");
  if (n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_nj: n must be < 2^31");
  if (src_kind != PPK_NJ_SQUARE && src_kind != PPK_NJ_LONG)
    return ppk_fail(PPK_ERR_ARG, "ppk_nj: src_kind must be PPK_NJ_SQUARE or PPK_NJ_LONG");
  if (src_kind == PPK_NJ_LONG && (stride == 0 || col >= stride))
    return ppk_fail(PPK_ERR_ARG, "ppk_nj: the long form needs col < stride");
  if (n > 1 && (!d_src || !d_join || !d_len)) return ppk_fail(PPK_ERR_ARG, "ppk_nj: NULL array");
  if (n == 1) return PPK_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);

  // scratch: bad | best slots | old_of | per-slot S, nd, ids, alive (x2) | triangle 0 | triangle 1
  const size_t c1 = first_compaction((long long)n);
  unsigned long long *bad;
  Best *part;
  unsigned *old_of;
  double *S[2], *nd[2], *W[2];
  long long *ids[2];
  unsigned char *alive[2];
  int rc = ppk_scratch_carve(dev, SLOT_NJ, [&](Carve &c) {
    c.take(bad, 1).take(part, kMaxParts).take(old_of, n);
    for (int i = 0; i < 2; ++i) c.take(S[i], n).take(nd[i], n).take(ids[i], n).take(alive[i], n);
    c.take(W[0], tri(n)).take(W[1], tri(c1));
  });
  if (rc != PPK_OK) return rc;

  // -- load: the one synchronisation
  ppk_prof_stage("load", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  hipLaunchKernelGGL(nj_load_kernel, dim3((unsigned)(n - 1 < 8192 ? n - 1 : 8192)), dim3(kThreads), 0, s, d_src,
                     src_kind, stride, col, n, W[0], bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 8}}, &h)) != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return nj_bad_entry(d_src, src_kind, stride, col, n, (size_t)h[0]);
  }
  ppk_prof_stage("rowsum", s);
  hipLaunchKernelGGL(nj_rowsum_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, W[0], n,
                     S[0], nd[0], ids[0], alive[0]);
  PPK_HIP(hipGetLastError());

  int cur = 0;
  long long r = (long long)n, m = (long long)n, t = 0;
  auto compact = [&]() -> int {
    ppk_prof_stage("compact", s);
    const int nx = cur ^ 1;
    hipLaunchKernelGGL(nj_compact_map_kernel, dim3(1), dim3(kTailThreads), 0, s, alive[cur], S[cur], nd[cur],
                       ids[cur], (size_t)m, old_of, S[nx], nd[nx], ids[nx], alive[nx]);
    hipLaunchKernelGGL(nj_compact_copy_kernel, dim3((unsigned)(r - 1 < 8192 ? r - 1 : 8192)), dim3(kThreads), 0, s,
                       W[cur], old_of, (size_t)r, W[nx]);
    PPK_HIP(hipGetLastError());
    cur = nx;
    m = r;
    return PPK_OK;
  };
  while (r > kTailR) {
    if (compact_due(r, m) && (rc = compact()) != PPK_OK) return rc;
    const unsigned g = scan_parts((size_t)m);
    const unsigned gu = (unsigned)((m + kThreads - 1) / kThreads < 64 ? (m + kThreads - 1) / kThreads : 64);
    ppk_prof_stage("scan", s);
    hipLaunchKernelGGL(nj_scan_kernel, dim3(g), dim3(kThreads), 0, s, W[cur], alive[cur], nd[cur], (size_t)m, part);
    ppk_prof_stage("update", s);
    hipLaunchKernelGGL(nj_update_kernel, dim3(gu), dim3(kThreads), 0, s, W[cur], alive[cur], S[cur], nd[cur],
                       ids[cur], part, g, (size_t)m, r, t, (long long)n, d_join, d_len);
    PPK_HIP(hipGetLastError());
    --r;
    ++t;
    if (t % kPoll == 0 && ppk_interrupted()) {
      ppk_prof_stage(nullptr, s);
      PPK_HIP(hipStreamSynchronize(s));
      return ppk_fail(PPK_ERR_INTERRUPTED, "ppk_nj: interrupted");
    }
  }
  if (m > r && (rc = compact()) != PPK_OK) return rc;
  ppk_prof_stage("tail", s);
  hipLaunchKernelGGL(nj_tail_kernel, dim3(1), dim3(kTailThreads), 0, s, W[cur], alive[cur], S[cur], nd[cur], ids[cur],
                     (size_t)m, r, t, (long long)n, d_join, d_len);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage(nullptr, s);
  return PPK_OK;
}

extern "C" int ppk_nj(const float *square, size_t n, int device_id, long long *join, double *len) {
  if (n == 0) return ppk_fail(PPK_ERR_ARG, "ppk_nj: n must be at least 1");
  if (n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, "ppk_nj: n must be < 2^31");
  if (n > 1 && (!square || !join || !len)) return ppk_fail(PPK_ERR_ARG, "ppk_nj: NULL array");
  if (n == 1) return PPK_OK;
  float *d_sq;
  long long *d_join;
  double *d_len;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_sq, n * n).take(d_join, 2 * (n - 1)).take(d_len, 2 * (n - 1));
  }, [&]() -> int {
    PPK_HIP(hipMemcpy(d_sq, square, n * n * 4, hipMemcpyHostToDevice));
    const int rc = ppk_nj_dev(d_sq, PPK_NJ_SQUARE, 1, 0, n, d_join, d_len, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(join, d_join, (n - 1) * 16, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(len, d_len, (n - 1) * 16, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// Mean distance of every cluster of a nested family in one pass over the matrix.
//
//  - ppk_cluster_pair_sums_dev : scripts/poppunk_iterate.py:184-197 asks pp_sketchlib.queryDatabase for the core
//    distances of every cluster of its family and takes their mean, so a pair is recomputed once per level that holds
//    it.  Here the condensed matrix is resident: every row (i, j) is read once and added to ONE bucket, (t*, c) = the
//    first level at which i and j share a cluster and that cluster's number; the host adds the buckets of a cluster's
//    sub-clusters (n_levels * n work).  The levels are nested, so "together at level t" is monotone in t and t* is found
//    by bisection, as the sweeps' classify pass does over its nested boundaries (ppk_iterate.hip).
//    Values are added as integers, llrint(x * 2^shift): integer addition is associative, so the sums are the same bits
//    whatever order the atomics land in.
//    Stages (ppk_prof_stages names):
//      levels    every cluster number checked against [1, n]
//      pairs     the streaming pass.  A workgroup owns chunks of consecutive rows; a thread derives (i, j) once per
//                chunk and steps along the condensed order.  Rows of one wave share i (or two) and have consecutive j,
//                so they usually fall in one or two buckets: up to two distinct buckets are summed across the wave
//                first, whatever is left goes lane by lane; all of it into a per-workgroup LDS table (direct-mapped on
//                a hash of the bucket, a slot claimed by compare-and-swap; a bucket that loses its slot goes to global
//                memory), which is flushed with one global atomic per used slot when the workgroup ends.
//    The call's ONE synchronisation reads the first bad row / bad cluster number.
#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 16;             // rows per thread of one chunk
constexpr int kSlots = 1024;           // LDS table entries (24 KiB)
constexpr int kMaxLevels = 1023;
constexpr unsigned long long kEmpty = ~0ull;

__global__ void __launch_bounds__(kThreads) ps_levels_kernel(const int32_t *levels, size_t count, long long n,
                                                             unsigned long long *bad) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (size_t)gridDim.x * blockDim.x) {
    const long long c = levels[k];
    if (c < 1 || c > n) atomicMin(bad, (unsigned long long)k);
  }
}

struct PsTable {
  unsigned long long key[kSlots], sum[kSlots], cnt[kSlots];
};

__device__ __forceinline__ void ps_add(PsTable &t, unsigned long long key, unsigned long long s, unsigned long long c,
                                       unsigned long long *g_sum, unsigned long long *g_cnt) {
  const unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 54);      // 10 bits
  const unsigned long long old = atomicCAS(&t.key[slot], kEmpty, key);
  if (old == kEmpty || old == key) {
    atomicAdd(&t.sum[slot], s);
    atomicAdd(&t.cnt[slot], c);
  } else {
    atomicAdd(&g_sum[key], s);
    atomicAdd(&g_cnt[key], c);
  }
}

// every lane of the wave calls this; key == kEmpty: nothing to add
__device__ __forceinline__ void ps_wave_add(PsTable &t, unsigned long long key, unsigned long long v,
                                            unsigned long long *g_sum, unsigned long long *g_cnt) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const unsigned long long pend = __ballot(key != kEmpty);
    if (!pend) return;                 // (wave-uniform)
    const int leader = __ffsll((long long)pend) - 1;
    const unsigned long long k0 = __shfl(key, leader);
    const bool mine = key == k0;
    const unsigned long long s = wave_sum_all(mine ? v : 0ull);
    const unsigned long long c = (unsigned long long)__popcll(__ballot(mine));
    if (lane == leader) ps_add(t, k0, s, c, g_sum, g_cnt);
    if (mine) key = kEmpty;
  }
  if (key != kEmpty) ps_add(t, key, v, 1, g_sum, g_cnt);
}

__global__ void __launch_bounds__(kThreads) ps_pairs_kernel(const float *dist, size_t n_rows, size_t n, int col,
                                                            const int32_t *levels, int n_levels, double scale,
                                                            unsigned long long *g_sum, unsigned long long *g_cnt,
                                                            unsigned long long *bad) {
  __shared__ PsTable table;
  for (int k = threadIdx.x; k < kSlots; k += blockDim.x) {
    table.key[k] = kEmpty;
    table.sum[k] = 0;
    table.cnt[k] = 0;
  }
  __syncthreads();
  const int32_t *last = levels + (size_t)(n_levels - 1) * n;
  const size_t chunk = (size_t)kThreads * kItems;
  for (size_t c0 = (size_t)blockIdx.x * chunk; c0 < n_rows; c0 += (size_t)gridDim.x * chunk) {
    size_t k = c0 + threadIdx.x, i = 0, j = 0;
    if (k < n_rows) {
      i = cond_row_i(k, n);
      j = i + 1 + (k - cond_row_start(i, n));
    }
    for (int q = 0; q < kItems; ++q) {
      unsigned long long key = kEmpty, v = 0;
      if (k < n_rows) {
        const float x = dist[2 * k + col];
        if (!(x >= 0.0f && x <= 1.0f)) {             // (NaN fails both)
          atomicMin(bad, (unsigned long long)k);
        } else if (last[i] == last[j]) {
          int lo = 0, hi = n_levels - 1;             // the first level with equal numbers lies in [lo, hi]
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (levels[(size_t)mid * n + i] == levels[(size_t)mid * n + j]) hi = mid;
            else lo = mid + 1;
          }
          const long long c = levels[(size_t)lo * n + i];
          if (c >= 1 && c <= (long long)n) {         // (ps_levels_kernel reports the others)
            key = (unsigned long long)lo * (n + 1) + (unsigned long long)c;
            v = (unsigned long long)__double2ll_rn((double)x * scale);
          }
        }
        k += kThreads;
        if (k < n_rows) {                            // step along the condensed order: i <= n - 2 exists for row k
          j += kThreads;
          while (j >= n) {
            ++i;
            j = j - n + i + 1;
          }
        }
      }
      ps_wave_add(table, key, v, g_sum, g_cnt);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kSlots; k += blockDim.x)
    if (table.key[k] != kEmpty) {
      atomicAdd(&g_sum[table.key[k]], table.sum[k]);
      atomicAdd(&g_cnt[table.key[k]], table.cnt[k]);
    }
}

const char *kWho = "ppk_cluster_pair_sums";

}  // namespace

extern "C" int ppk_cluster_pair_sums_dev(const float *d_dist, size_t n_rows, int col, const int32_t *d_levels,
                                         size_t n_levels, int shift, long long *d_sum, long long *d_cnt,
                                         void *stream) {
  const std::string who = kWho;
  if (col != 0 && col != 1) return ppk_fail(PPK_ERR_ARG, who + ": col must be 0 or 1");
  if (shift < 0 || shift > 40) return ppk_fail(PPK_ERR_ARG, who + ": shift must be 0 .. 40");
  if (n_levels == 0 || n_levels > (size_t)kMaxLevels) return ppk_fail(PPK_ERR_ARG, who + ": n_levels must be 1 .. 1023");
  size_t n = 0;
  const int rc0 = ppk_condensed_samples(n_rows, &n, who + ": ");
  if (rc0 != PPK_OK) return rc0;
  if (n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n must be < 2^31");
  if (shift > 62 - ceil_log2(n_rows ? n_rows : 1))
    return ppk_fail(PPK_ERR_ARG, who + ": shift must be at most 62 - ceil_log2(n_rows), or a sum could pass 2^62");
  if (!d_levels || !d_sum || !d_cnt || (n_rows && !d_dist)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  unsigned long long *bad;
  int rc = ppk_scratch_carve(dev, SLOT_CLUSTERS, [&](Carve &c) { c.take(bad, 2); });
  if (rc != PPK_OK) return rc;
  const size_t buckets = n_levels * (n + 1);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 16, s));
  PPK_HIP(hipMemsetAsync(d_sum, 0, buckets * 8, s));
  PPK_HIP(hipMemsetAsync(d_cnt, 0, buckets * 8, s));
  ppk_prof_stage("levels", s);
  hipLaunchKernelGGL(ps_levels_kernel, dim3(grid_for(n_levels * n, kThreads * 4, 2048)), dim3(kThreads), 0, s, d_levels,
                     n_levels * n, (long long)n, bad + 1);
  ppk_prof_stage("pairs", s);
  if (n_rows)
    hipLaunchKernelGGL(ps_pairs_kernel, dim3(grid_for(n_rows, (size_t)kThreads * kItems, 4096)), dim3(kThreads), 0, s,
                       d_dist, n_rows, n, col, d_levels, (int)n_levels, std::ldexp(1.0, shift),
                       reinterpret_cast<unsigned long long *>(d_sum), reinterpret_cast<unsigned long long *>(d_cnt), bad);
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 16}}, &h)) != PPK_OK) return rc;
  if (h[1] != ~0ull) {
    const size_t k = (size_t)h[1];
    int32_t c = 0;
    PPK_HIP(hipMemcpy(&c, d_levels + k, 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": level " + std::to_string(k / n) + ", vertex " + std::to_string(k % n) +
                                     ": cluster number " + std::to_string(c) + " outside [1, " + std::to_string(n) + "]");
  }
  if (h[0] != ~0ull) {
    const size_t k = (size_t)h[0];
    float x = 0.0f;
    PPK_HIP(hipMemcpy(&x, d_dist + 2 * k + col, 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": row " + std::to_string(k) + ": value " + std::to_string(x) +
                                     " is not a finite number in [0, 1]");
  }
  return PPK_OK;
}

extern "C" int ppk_cluster_pair_sums(const float *dist, size_t n_rows, int col, const int32_t *levels, size_t n_levels,
                                     int shift, int device_id, long long *sum, long long *cnt) {
  const std::string who = kWho;
  if (!levels || !sum || !cnt || (n_rows && !dist)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (n_levels == 0 || n_levels > (size_t)kMaxLevels) return ppk_fail(PPK_ERR_ARG, who + ": n_levels must be 1 .. 1023");
  size_t n = 0;
  const int rc0 = ppk_condensed_samples(n_rows, &n, who + ": ");
  if (rc0 != PPK_OK) return rc0;
  const size_t buckets = n_levels * (n + 1);
  float *d_dist;
  int32_t *d_levels;
  long long *d_sum, *d_cnt;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_dist, 2 * n_rows).take(d_levels, n_levels * n).take(d_sum, buckets).take(d_cnt, buckets);
  }, [&]() -> int {
    if (n_rows) PPK_HIP(hipMemcpy(d_dist, dist, n_rows * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_levels, levels, n_levels * n * 4, hipMemcpyHostToDevice));
    const int rc = ppk_cluster_pair_sums_dev(d_dist, n_rows, col, d_levels, n_levels, shift, d_sum, d_cnt, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(sum, d_sum, buckets * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(cnt, d_cnt, buckets * 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// Silhouette of every sample under every level of a family of clusterings, from the resident matrix.
//
//  - ppk_silhouette_dev : scripts/poppunk_calculate_silhouette.py builds an n x n float64 matrix from the long-form
//    distances in a Python loop and hands it to sklearn.metrics.silhouette_score(metric='precomputed'), one clustering
//    per run.  Here the condensed matrix is resident and never squared: samples are taken in bands, a band's rows are
//    laid out as float32 [band][n] of the chosen metric, and one workgroup per (sample, level) adds its row into a table
//    indexed by label.  Distances are added as integers, llrint(d * 2^shift): integer addition is associative, so
//    T[i][c] is the same bits whatever order the atomics land in, and a, b, s follow from it in float64 by the
//    operations include/ppk.h lists (tests/silhouette_model.py restates them in numpy and is met bit for bit).
//    Stages (ppk_prof_stages names):
//      check   both columns of every row against [0, 1], every label against [1, n]; the same pass counts the samples
//              of every (level, label), then one workgroup per level counts its distinct labels and finds the largest.
//              The call's ONE synchronisation reads the first bad row / bad label here, before a label indexes anything.
//      band    rows [i0, i1) of the square into scratch, 64 x 64 tiles: columns j > i are contiguous in condensed row i
//              and go straight through; columns j < i are read row j at a time (samples i0 .. i0 + 63 are contiguous
//              there) and transposed in LDS, so both triangles are read with coalesced rows.
//      sums    one workgroup per (sample, level), levels innermost, so a band is re-read while it is in the Infinity
//              Cache.  The row is streamed with 16-byte loads; lanes of a wave that share a label are summed across the
//              wave first (two rounds, as ps_wave_add of ppk_clusters.hip), the rest goes lane by lane, all of it into
//              an LDS table of int64 slots.  Labels beyond the table are taken in further windows over the same row
//              (in L2 by then); after each window the slots reduce to a running minimum of T / cnt over the other
//              labels, and the sample's own slot is picked up.  No window starts beyond the level's largest label.
#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kWindowMax = 4096;       // int64 slots of the label table (32 KiB: four workgroups per CU)
constexpr int kMaxLevels = 1023;

// the distance of one row of the matrix: float32, nothing fused
__device__ __forceinline__ float sil_metric(float x0, float x1, int metric) {
  if (metric == 0) return x0;
  if (metric == 1) return x1;
  if (metric == 2) return ppk_euclid(x0, x1);
  return fabsf(__fsub_rn(x0, x1));
}

__global__ void __launch_bounds__(kThreads) sil_check_dist_kernel(const float *dist, size_t n_rows,
                                                                  unsigned long long *bad) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += (size_t)gridDim.x * blockDim.x) {
    const float x0 = dist[2 * k], x1 = dist[2 * k + 1];
    if (!(x0 >= 0.0f && x0 <= 1.0f && x1 >= 0.0f && x1 <= 1.0f)) atomicMin(bad, (unsigned long long)k);   // (NaN fails)
  }
}

// cnt int32 [n_levels][n + 1], zeroed by the caller
__global__ void __launch_bounds__(kThreads) sil_labels_kernel(const int32_t *labels, size_t count, size_t n,
                                                              int32_t *cnt, unsigned long long *bad) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < count; k += (size_t)gridDim.x * blockDim.x) {
    const long long c = labels[k];
    if (c < 1 || c > (long long)n) atomicMin(bad, (unsigned long long)k);
    else atomicAdd(&cnt[(k / n) * (n + 1) + (size_t)c], 1);
  }
}

// one workgroup per level: the distinct labels, the largest of them, and check_number_of_labels
__global__ void __launch_bounds__(kThreads) sil_levels_kernel(const int32_t *cnt, size_t n, int32_t *n_labels,
                                                              int32_t *valid, int32_t *max_label) {
  __shared__ int s_count, s_max;
  if (threadIdx.x == 0) s_count = s_max = 0;
  __syncthreads();
  const int32_t *row = cnt + (size_t)blockIdx.x * (n + 1);
  int count = 0, top = 0;
  for (size_t c = 1 + threadIdx.x; c <= n; c += kThreads)
    if (row[c] > 0) {
      ++count;
      top = (int)c;
    }
  atomicAdd(&s_count, count);
  atomicMax(&s_max, top);
  __syncthreads();
  if (threadIdx.x == 0) {
    n_labels[blockIdx.x] = s_count;
    valid[blockIdx.x] = (s_count >= 2 && (size_t)s_count + 1 <= n) ? 1 : 0;
    max_label[blockIdx.x] = s_max;
  }
}

// grid: (n / 64 column tiles) x (band / 64 row tiles).  out float32 [i1 - i0][ld], the diagonal 0.
__global__ void __launch_bounds__(kThreads) sil_band_kernel(const float *__restrict__ dist, size_t n, int metric,
                                                            size_t i0, size_t i1, size_t ld, float *__restrict__ out) {
  __shared__ float tile[kTile][kTile + 1];
  const size_t ib = i0 + (size_t)blockIdx.y * kTile, jb = (size_t)blockIdx.x * kTile;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 64 x 4
  if (jb + kTile > ib) {                 // the tile holds columns j >= i: condensed row i, contiguous in j
    for (int r = ty; r < kTile; r += 4) {
      const size_t i = ib + r, j = jb + tx;
      if (i < i1 && j < n && j >= i) {
        float v = 0.0f;
        if (j > i) {
          const size_t k = cond_index(i, j, n);
          v = sil_metric(dist[2 * k], dist[2 * k + 1], metric);
        }
        out[(i - i0) * ld + j] = v;
      }
    }
  }
  if (jb < ib + kTile - 1) {             // ... and columns j < i: condensed row j, contiguous in i (block-uniform)
    for (int r = ty; r < kTile; r += 4) {
      const size_t j = jb + r, i = ib + tx;
      if (i < i1 && j < i) {
        const size_t k = cond_index(j, i, n);
        tile[r][tx] = sil_metric(dist[2 * k], dist[2 * k + 1], metric);
      }
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += 4) {
      const size_t i = ib + r, j = jb + tx;
      if (i < i1 && j < i) out[(i - i0) * ld + j] = tile[tx][r];
    }
  }
}

// every lane of the wave calls this; key < 0: nothing to add
__device__ __forceinline__ void sil_wave_add(unsigned long long *table, int key, unsigned long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const unsigned long long pend = __ballot(key >= 0);
    if (!pend) return;                   // (wave-uniform)
    const int leader = __ffsll((long long)pend) - 1;
    const int k0 = __shfl(key, leader);
    const bool mine = key == k0;
    if (__popcll(__ballot(mine)) == 1) { // (wave-uniform) a label of its own: nothing to sum
      if (mine) atomicAdd(&table[k0], v);
    } else {
      const unsigned long long s = wave_sum_all(mine ? v : 0ull);
      if (lane == leader) atomicAdd(&table[k0], s);
    }
    if (mine) key = -1;
  }
  if (key >= 0) atomicAdd(&table[key], v);
}

__device__ __forceinline__ void sil_store(double *a_out, double *b_out, double *s_out, size_t o, double a, double b,
                                          double s) {
  if (a_out) a_out[o] = a;
  if (b_out) b_out[o] = b;
  s_out[o] = s;
}

// grid: (i1 - i0) * n_levels workgroups, levels innermost
__global__ void __launch_bounds__(kThreads) sil_sums_kernel(const float *__restrict__ band, size_t ld, size_t n,
                                                            size_t i0, const int32_t *__restrict__ labels, int n_levels,
                                                            const int32_t *__restrict__ cnt,
                                                            const int32_t *__restrict__ valid,
                                                            const int32_t *__restrict__ max_label, int window,
                                                            double scale, double inv_scale, double *a_out,
                                                            double *b_out, double *s_out) {
  __shared__ unsigned long long table[kWindowMax];
  __shared__ unsigned long long own_sum;
  __shared__ double wave_min[kThreads / 64];
  const int t = (int)(blockIdx.x % (unsigned)n_levels);
  const size_t i = i0 + blockIdx.x / (unsigned)n_levels;
  const size_t o = (size_t)t * n + i;
  const int32_t *lab = labels + (size_t)t * n;
  const int32_t *cn = cnt + (size_t)t * (n + 1);
  const long long ci = lab[i];
  // (all three are workgroup-uniform)
  if (!valid[t] || ci < 1 || ci > (long long)n) {
    if (threadIdx.x == 0) sil_store(a_out, b_out, s_out, o, NAN, NAN, NAN);
    return;
  }
  const int own = cn[ci];
  if (own == 1) {
    if (threadIdx.x == 0) sil_store(a_out, b_out, s_out, o, 0.0, 0.0, 0.0);
    return;
  }
  const float *row = band + (i - i0) * ld;
  const long long top = max_label[t];
  double best = INFINITY;
  if (threadIdx.x == 0) own_sum = 0;
  for (long long w0 = 1; w0 <= top; w0 += window) {
    const int wlen = (int)(top - w0 + 1 < (long long)window ? top - w0 + 1 : (long long)window);
    for (int k = threadIdx.x; k < wlen; k += kThreads) table[k] = 0;
    __syncthreads();
    for (size_t base = 0; base < n; base += (size_t)kThreads * 4) {
      const size_t j4 = base + (size_t)threadIdx.x * 4;
      float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (j4 < n) x = *reinterpret_cast<const float4 *>(row + j4);     // (j4 + 3 < ld: ld is a multiple of 4)
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int key = -1;
        unsigned long long v = 0;
        if (j4 + e < n) {
          const long long k = (long long)lab[j4 + e] - w0;
          if (k >= 0 && k < (long long)wlen) {
            key = (int)k;
            v = (unsigned long long)__double2ll_rn((double)xs[e] * scale);   // (the diagonal holds 0 and adds 0)
          }
        }
        sil_wave_add(table, key, v);
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < wlen; k += kThreads) {
      const long long c = w0 + k;
      const int m = cn[c];
      if (m <= 0) continue;
      if (c == ci) {
        own_sum = table[k];
      } else {
        const double mean = ((double)(long long)table[k] * inv_scale) / (double)m;
        best = mean < best ? mean : best;
      }
    }
    __syncthreads();
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double other = __shfl_xor(best, off);
    best = other < best ? other : best;
  }
  if ((threadIdx.x & 63) == 0) wave_min[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = wave_min[0];
    for (int w = 1; w < kThreads / 64; ++w) b = wave_min[w] < b ? wave_min[w] : b;
    const double a = ((double)(long long)own_sum * inv_scale) / (double)(own - 1);
    const double top_ab = a > b ? a : b;
    const double s = top_ab == 0.0 ? 0.0 : (b - a) / top_ab;
    sil_store(a_out, b_out, s_out, o, a, b, s);
  }
}

const char *kWho = "ppk_silhouette";

// the argument errors that need no device; *n: the samples
int sil_check_args(size_t n_rows, int metric, size_t n_levels, int shift, size_t *n) {
  const std::string who = kWho;
  if (metric < 0 || metric > 3) return ppk_fail(PPK_ERR_ARG, who + ": metric must be 0 .. 3");
  if (shift < 0 || shift > 40) return ppk_fail(PPK_ERR_ARG, who + ": shift must be 0 .. 40");
  if (n_levels == 0 || n_levels > (size_t)kMaxLevels) return ppk_fail(PPK_ERR_ARG, who + ": n_levels must be 1 .. 1023");
  const int rc = ppk_condensed_samples(n_rows, n, who + ": ");
  if (rc != PPK_OK) return rc;
  if (*n < 3) return ppk_fail(PPK_ERR_ARG, who + ": n must be at least 3");
  if (*n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n must be < 2^31");
  if (shift > 61 - ceil_log2(*n))
    return ppk_fail(PPK_ERR_ARG, who + ": shift must be at most 61 - ceil_log2(n), or a sum could pass 2^62");
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_silhouette_dev(const float *d_dist, size_t n_rows, int metric, const int32_t *d_labels,
                                  size_t n_levels, int shift, double *d_a, double *d_b, double *d_s,
                                  int32_t *d_n_labels, int32_t *d_valid, void *stream) {
  const std::string who = kWho;
  size_t n = 0;
  int rc = sil_check_args(n_rows, metric, n_levels, shift, &n);
  if (rc != PPK_OK) return rc;
  if (!d_dist || !d_labels || !d_s || !d_n_labels || !d_valid) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);

  // the band: rows of ld floats (16-byte rows), as many as four fifths of the cap hold (a scratch slot is allocated
  // with a quarter to spare, and the cap is on what is allocated); a launch holds fewer than 2^31 workgroups
  const size_t ld = (n + 3) & ~(size_t)3;
  const long long cap_mb = ppk_config().silhouette_scratch_mb.load();
  size_t band = ((size_t)(cap_mb > 0 ? cap_mb : 0) << 20) / 5 * 4 / (ld * sizeof(float));
  if (const long long force = ppk_config().silhouette_band.load(); force > 0) band = (size_t)force;
  if (band < 1) band = 1;
  if (band > n) band = n;
  if (band > (((size_t)1 << 31) - 1) / n_levels) band = (((size_t)1 << 31) - 1) / n_levels;
  if (band > (size_t)65535 * kTile) band = (size_t)65535 * kTile;       // (the band kernel's grid rows)
  long long window = ppk_config().silhouette_window.load();
  if (window < 1 || window > kWindowMax) window = kWindowMax;

  unsigned long long *bad;
  int32_t *cnt, *max_label;
  float *rows;
  rc = ppk_scratch_carve(dev, SLOT_SILHOUETTE, [&](Carve &c) {
    c.take(bad, 2).take(max_label, n_levels).take(cnt, n_levels * (n + 1)).take(rows, band * ld);
  });
  if (rc != PPK_OK) return rc;

  ppk_prof_stage("check", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 16, s));
  PPK_HIP(hipMemsetAsync(cnt, 0, n_levels * (n + 1) * sizeof(int32_t), s));
  hipLaunchKernelGGL(sil_check_dist_kernel, dim3(grid_for(n_rows, kThreads * 8, 4096)), dim3(kThreads), 0, s, d_dist,
                     n_rows, bad);
  hipLaunchKernelGGL(sil_labels_kernel, dim3(grid_for(n_levels * n, kThreads * 4, 2048)), dim3(kThreads), 0, s,
                     d_labels, n_levels * n, n, cnt, bad + 1);
  hipLaunchKernelGGL(sil_levels_kernel, dim3((unsigned)n_levels), dim3(kThreads), 0, s, cnt, n, d_n_labels, d_valid,
                     max_label);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  rc = ppk_read_back(dev, s, {{bad, 16}}, &h);
  ppk_prof_stage(nullptr, s);
  if (rc != PPK_OK) return rc;
  if (h[1] != ~0ull) {
    const size_t k = (size_t)h[1];
    int32_t c = 0;
    PPK_HIP(hipMemcpy(&c, d_labels + k, 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": level " + std::to_string(k / n) + ", vertex " + std::to_string(k % n) +
                                     ": label " + std::to_string(c) + " outside [1, " + std::to_string(n) + "]");
  }
  if (h[0] != ~0ull) {
    const size_t k = (size_t)h[0];
    float x[2] = {0.0f, 0.0f};
    PPK_HIP(hipMemcpy(x, d_dist + 2 * k, 8, hipMemcpyDeviceToHost));
    const int col = (x[0] >= 0.0f && x[0] <= 1.0f) ? 1 : 0;
    return ppk_fail(PPK_ERR_ARG, who + ": row " + std::to_string(k) + ", column " + std::to_string(col) + ": value " +
                                     std::to_string(x[col]) + " is not a finite number in [0, 1]");
  }

  const double scale = std::ldexp(1.0, shift), inv_scale = std::ldexp(1.0, -shift);
  for (size_t i0 = 0; i0 < n; i0 += band) {
    const size_t i1 = i0 + band < n ? i0 + band : n;
    ppk_prof_stage("band", s);
    hipLaunchKernelGGL(sil_band_kernel, dim3((unsigned)((n + kTile - 1) / kTile), (unsigned)((i1 - i0 + kTile - 1) / kTile)),
                       dim3(kThreads), 0, s, d_dist, n, metric, i0, i1, ld, rows);
    ppk_prof_stage("sums", s);
    hipLaunchKernelGGL(sil_sums_kernel, dim3((unsigned)((i1 - i0) * n_levels)), dim3(kThreads), 0, s, rows, ld, n, i0,
                       d_labels, (int)n_levels, cnt, d_valid, max_label, (int)window, scale, inv_scale, d_a, d_b, d_s);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

extern "C" int ppk_silhouette(const float *dist, size_t n_rows, int metric, const int32_t *labels, size_t n_levels,
                              int shift, int device_id, double *a, double *b, double *s, int32_t *n_labels,
                              int32_t *valid) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const std::string who = kWho;
  size_t n = 0;
  const int rc0 = sil_check_args(n_rows, metric, n_levels, shift, &n);
  if (rc0 != PPK_OK) return rc0;
  if (!dist || !labels || !s || !n_labels || !valid) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const size_t cells = n_levels * n;
  float *d_dist;
  int32_t *d_labels, *d_n_labels, *d_valid;
  double *d_a, *d_b, *d_s;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_dist, 2 * n_rows).take(d_labels, cells).take(d_a, a ? cells : 0).take(d_b, b ? cells : 0).take(d_s, cells)
        .take(d_n_labels, n_levels).take(d_valid, n_levels);
  }, [&]() -> int {
    PPK_HIP(hipMemcpy(d_dist, dist, n_rows * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_labels, labels, cells * 4, hipMemcpyHostToDevice));
    const int rc = ppk_silhouette_dev(d_dist, n_rows, metric, d_labels, n_levels, shift, a ? d_a : nullptr,
                                      b ? d_b : nullptr, d_s, d_n_labels, d_valid, nullptr);
    if (rc != PPK_OK) return rc;
    if (a) PPK_HIP(hipMemcpy(a, d_a, cells * 8, hipMemcpyDeviceToHost));
    if (b) PPK_HIP(hipMemcpy(b, d_b, cells * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(s, d_s, cells * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(n_labels, d_n_labels, n_levels * 4, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(valid, d_valid, n_levels * 4, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// Density grids of a resident [rows][2] matrix: the two layers of the fit plots.
//
//  - ppk_density_kde_dev : PopPUNK/plot.py:62-66 fits an Epanechnikov KernelDensity (ball tree) to at most 1 000 000
//    sampled rows and scores it on a 100 x 100 grid.  The kernel has compact support, so a row reaches only the nodes
//    within h of it: every row read adds llrint((1 - d^2 / h^2) * 2^shift) to those nodes, as integers, so the sums are
//    the same bits whatever order the atomics land in (ppk_clusters.hip's pair sums are the same kind of pass).
//    Stages (ppk_prof_stages names):
//      scale     (scale NULL only) the column maxima of the rows read, as order-preserving keys
//      kde       the streaming pass.  A workgroup keeps a private copy of the grid (int64) and of the node coordinates
//                in LDS; a thread takes one row at a time, finds its window of nodes by bisection over the coordinates
//                and adds with LDS atomics; when its chunks are done the workgroup flushes the non-zero cells with one
//                global 64-bit atomic each.  Option "density_kde_presum" (0: off) sums the terms of lanes that share a
//                window across the wave first (dn_presum); same sums.
//  - ppk_density_counts_dev : plot_results / plot_dbscan_results / plot_refined_results hand matplotlib one marker per
//    row (plot.py:221, :275, :330-331).  What reaches the picture is which pixels hold a row of which label: one pass,
//    one 32-bit atomic per row, through a per-workgroup LDS table of hot pixels (direct-mapped on a hash of the cell, a
//    slot claimed by compare-and-swap; a cell that loses its slot goes to global memory) -- option "density_hot_table".
//    Stage: counts.
//  Each call's ONE synchronisation reads the first offenders (and the scale).
#include <cmath>
#include <cstdio>
#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 16;                   // rows per thread of one chunk
constexpr int kHotSlots = 1024;              // entries of the counts pass's LDS table (8 KiB)
constexpr unsigned kEmpty = ~0u;
constexpr size_t kKdeLdsDefault = 65536 - 64;      // what a kernel gets without the opt-in

__device__ __forceinline__ void dn_row(const float *dist, size_t r, bool aligned, float &x, float &y) {
  if (aligned) {
    const float2 p = reinterpret_cast<const float2 *>(dist)[r];
    x = p.x;
    y = p.y;
  } else {
    x = dist[2 * r];
    y = dist[2 * r + 1];
  }
}
__device__ __forceinline__ bool dn_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // (NaN fails)

__global__ void dn_set_scale_kernel(unsigned *keys, unsigned k0, unsigned k1) {
  keys[0] = k0;
  keys[1] = k1;
}

// the column maxima of the rows read, as ord_of keys (keys zeroed by the caller: below every float's key)
__global__ void __launch_bounds__(kThreads) dn_scale_kernel(const float *dist, size_t n_rows, const long long *idx,
                                                            size_t n_read, unsigned *keys) {
  const bool aligned = (reinterpret_cast<uintptr_t>(dist) & 7) == 0;
  unsigned m0 = 0, m1 = 0;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_read; k += (size_t)gridDim.x * blockDim.x) {
    size_t r = k;
    if (idx) {
      const long long v = idx[k];
      if (v < 0 || (unsigned long long)v >= n_rows) continue;      // (the kde pass reports it)
      r = (size_t)v;
    }
    float x, y;
    dn_row(dist, r, aligned, x, y);
    const unsigned k0 = ord_of(x), k1 = ord_of(y);
    m0 = k0 > m0 ? k0 : m0;
    m1 = k1 > m1 ? k1 : m1;
  }
  for (int o = PPK_LANES / 2; o > 0; o >>= 1) {
    const unsigned o0 = __shfl_xor(m0, o), o1 = __shfl_xor(m1, o);
    m0 = o0 > m0 ? o0 : m0;
    m1 = o1 > m1 ? o1 : m1;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&keys[0], m0);
    atomicMax(&keys[1], m1);
  }
}

// the first index with g[index] >= v (strict: > v); n when there is none.  A NaN v gives 0 from both.
template <bool STRICT>
__device__ __forceinline__ int dn_bound(const double *g, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (STRICT ? g[mid] <= v : g[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The wave pre-sum of the kde pass (option "density_kde_presum", the smallest group it serves; every lane of the wave
// calls this).  Rows with the same window of nodes visit the same cells in the same order, so a group of lanes that
// share a window can sum each cell's terms across the wave and add once.  The leader's window is broadcast
// (ballot-on-leader, as ps_wave_add); a group of at least `min_group` lanes is summed here and retired, a smaller one
// is left to its lanes.  At most kPresumRounds windows are looked at.  Returns whether this lane's row is still to add.
constexpr int kPresumRounds = 4;
__device__ __forceinline__ bool dn_presum(bool valid, int min_group, int a0, int a1, int b0, int b1, double px, double py,
                                          const double *lx, const double *ly, int ny, double inv_h2, double fix,
                                          unsigned long long *cell) {
  const int lane = threadIdx.x & 63;
  // (a window's ends are at most nx, ny <= PPK_DENSITY_KDE_MAX_CELLS < 2^16)
  const unsigned long long key = ((unsigned long long)a0 << 48) | ((unsigned long long)a1 << 32) |
                                 ((unsigned long long)b0 << 16) | (unsigned long long)b1;
  unsigned long long todo = __ballot(valid && a0 < a1 && b0 < b1);
  for (int round = 0; round < kPresumRounds && todo; ++round) {      // (wave-uniform)
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned long long k0 = __shfl(key, leader);
    const bool mine = ((todo >> lane) & 1) != 0 && key == k0;
    const unsigned long long grp = __ballot(mine);
    todo &= ~grp;
    if (__popcll(grp) < min_group) continue;
    const int wa0 = (int)(k0 >> 48), wa1 = (int)((k0 >> 32) & 0xffff);
    const int wb0 = (int)((k0 >> 16) & 0xffff), wb1 = (int)(k0 & 0xffff);
    for (int a = wa0; a < wa1; ++a) {
      const double dx = px - lx[a];
      const double dx2 = dx * dx;
      for (int b = wb0; b < wb1; ++b) {
        const double dy = py - ly[b];
        const double d2 = dx2 + dy * dy;
        const double t = 1.0 - d2 * inv_h2;
        // (each term < 2^40 and there are 64: the wave's sum is far below 2^62)
        const unsigned long long v = wave_sum(mine && t > 0.0 ? (unsigned long long)__double2ll_rn(t * fix) : 0ull);
        if (lane == 0 && v) atomicAdd(&cell[a * ny + b], v);
      }
    }
    if (mine) valid = false;
  }
  return valid;
}

// dynamic LDS: unsigned long long cell[nx * ny], double lx[nx], double ly[ny]
template <bool PRESUM>
__global__ void __launch_bounds__(kThreads) dn_kde_kernel(const float *dist, size_t n_rows, const long long *idx,
                                                          size_t n_read, const unsigned *scale_key, const double *gx,
                                                          int nx, const double *gy, int ny, double hw, double inv_h2,
                                                          double fix, int min_group, unsigned long long *g_sum,
                                                          unsigned long long *bad) {
  extern __shared__ unsigned long long dn_lds[];
  const int cells = nx * ny;
  unsigned long long *cell = dn_lds;
  double *lx = reinterpret_cast<double *>(dn_lds + cells), *ly = lx + nx;
  for (int c = threadIdx.x; c < cells; c += kThreads) cell[c] = 0;
  for (int c = threadIdx.x; c < nx; c += kThreads) lx[c] = gx[c];
  for (int c = threadIdx.x; c < ny; c += kThreads) ly[c] = gy[c];
  __syncthreads();
  const float s0 = ord_inv(scale_key[0]), s1 = ord_inv(scale_key[1]);
  const bool aligned = (reinterpret_cast<uintptr_t>(dist) & 7) == 0;
  const size_t chunk = (size_t)kThreads * kItems;
  for (size_t c0 = (size_t)blockIdx.x * chunk; c0 < n_read; c0 += (size_t)gridDim.x * chunk) {
    for (int q = 0; q < kItems; ++q) {
      const size_t k = c0 + (size_t)q * kThreads + threadIdx.x;
      if (!PRESUM && k >= n_read) break;
      if (PRESUM && c0 + (size_t)q * kThreads + (threadIdx.x & ~63) >= n_read) break;      // (the whole wave)
      bool valid = k < n_read;
      size_t r = k;
      if (valid && idx) {
        const long long v = idx[k];
        if (v < 0 || (unsigned long long)v >= n_rows) {
          atomicMin(bad, (unsigned long long)k);
          valid = false;
        }
        r = (size_t)v;
      }
      float x = 0.0f, y = 0.0f;
      if (valid) {
        dn_row(dist, r, aligned, x, y);
        if (!dn_finite(x) || !dn_finite(y)) {
          atomicMin(bad + 1, (unsigned long long)k);
          valid = false;
        }
      }
      double px = 0.0, py = 0.0;
      int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
      if (valid) {
        px = ppk_scaled_f32(x, s0);
        py = ppk_scaled_f32(y, s1);
        // Every node with t > 0 has |px - gx[a]| < h (1 + 1e-15) < hw, and rounding is monotone, so gx[a] > px - hw in
        // the reals gives gx[a] >= fl(px - hw): the window below holds all of them (likewise above, and for gy).
        a0 = dn_bound<false>(lx, nx, px - hw);
        a1 = dn_bound<true>(lx, nx, px + hw);
        b0 = dn_bound<false>(ly, ny, py - hw);
        b1 = dn_bound<true>(ly, ny, py + hw);
      }
      if (PRESUM) valid = dn_presum(valid, min_group, a0, a1, b0, b1, px, py, lx, ly, ny, inv_h2, fix, cell);
      if (!valid) continue;
      for (int a = a0; a < a1; ++a) {
        const double dx = px - lx[a];
        const double dx2 = dx * dx;
        for (int b = b0; b < b1; ++b) {
          const double dy = py - ly[b];
          const double d2 = dx2 + dy * dy;
          const double t = 1.0 - d2 * inv_h2;
          if (t > 0.0) atomicAdd(&cell[a * ny + b], (unsigned long long)__double2ll_rn(t * fix));
        }
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += kThreads)
    if (cell[c]) atomicAdd(&g_sum[c], cell[c]);
}

struct DnTable {
  unsigned key[kHotSlots], cnt[kHotSlots];
};

template <bool TABLE>
__global__ void __launch_bounds__(kThreads) dn_counts_kernel(const float *dist, size_t n_rows, const int32_t *label,
                                                             int label_lo, int n_slots, double x0, double inv_dx,
                                                             int nx, double y0, double inv_dy, int ny,
                                                             unsigned *counts, unsigned long long *outside,
                                                             unsigned long long *bad) {
  __shared__ DnTable table;
  if (TABLE) {
    for (int k = threadIdx.x; k < kHotSlots; k += kThreads) {
      table.key[k] = kEmpty;
      table.cnt[k] = 0;
    }
    __syncthreads();
  }
  const bool aligned = (reinterpret_cast<uintptr_t>(dist) & 7) == 0;
  unsigned long long out = 0;
  const size_t chunk = (size_t)kThreads * kItems;
  for (size_t c0 = (size_t)blockIdx.x * chunk; c0 < n_rows; c0 += (size_t)gridDim.x * chunk) {
    for (int q = 0; q < kItems; ++q) {
      const size_t k = c0 + (size_t)q * kThreads + threadIdx.x;
      if (k >= n_rows) break;
      float x, y;
      dn_row(dist, k, aligned, x, y);
      if (!dn_finite(x) || !dn_finite(y)) {
        atomicMin(bad, (unsigned long long)k);
        continue;
      }
      int slot = 0;
      if (label) {
        const long long l = (long long)label[k] - (long long)label_lo;
        if (l < 0 || l >= (long long)n_slots) {
          atomicMin(bad + 1, (unsigned long long)k);
          continue;
        }
        slot = (int)l;
      }
      const double fx = floor(((double)x - x0) * inv_dx), fy = floor(((double)y - y0) * inv_dy);
      if (!(fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny)) {
        ++out;
        continue;
      }
      const unsigned c = (unsigned)((slot * ny + (int)fy) * nx + (int)fx);      // < 2^26
      if (TABLE) {
        const unsigned h = (c * 0x9E3779B9u) >> 22;      // 10 bits
        const unsigned old = atomicCAS(&table.key[h], kEmpty, c);
        if (old == kEmpty || old == c) atomicAdd(&table.cnt[h], 1u);
        else atomicAdd(&counts[c], 1u);
      } else {
        atomicAdd(&counts[c], 1u);
      }
    }
  }
  wave_add(outside, out);
  if (TABLE) {
    __syncthreads();
    for (int k = threadIdx.x; k < kHotSlots; k += kThreads)
      if (table.key[k] != kEmpty) atomicAdd(&counts[table.key[k]], table.cnt[k]);
  }
}

const char *kWhoKde = "ppk_density_kde";
const char *kWhoCounts = "ppk_density_counts";

bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

std::string num(double v) {
  char buf[64];
  snprintf(buf, sizeof buf, "%g", v);
  return buf;
}

int kde_check_grid(const std::string &who, const char *name, const double *g, size_t n) {
  for (size_t a = 0; a < n; ++a) {
    if (!std::isfinite(g[a])) return ppk_fail(PPK_ERR_ARG, who + ": " + name + "[" + std::to_string(a) + "] is not finite");
    if (a && !(g[a] > g[a - 1]))
      return ppk_fail(PPK_ERR_ARG, who + ": " + name + " is not strictly ascending at index " + std::to_string(a));
  }
  return PPK_OK;
}

// every check of ppk_density_kde_dev that needs no device
int kde_check_args(size_t n_read, const float *scale, const double *gx, size_t nx, const double *gy, size_t ny, double h,
                   int shift, size_t limit) {
  const std::string who = kWhoKde;
  if (!gx || !gy) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  if (nx == 0 || ny == 0 || nx > limit || ny > limit || nx * ny + nx + ny > limit)
    return ppk_fail(PPK_ERR_ARG, who + ": nx * ny + nx + ny must be 1 .. " + std::to_string(limit) + " (a workgroup keeps the " +
                                     "grid and its coordinates in LDS; 100 x 100 " +
                                     (100 * 100 + 200 <= limit ? "fits" : "does not fit in the LDS this device grants") +
                                     "), got nx = " + std::to_string(nx) + ", ny = " + std::to_string(ny));
  if (shift < 0 || shift > 40) return ppk_fail(PPK_ERR_ARG, who + ": shift must be 0 .. 40");
  if (shift > 62 - ceil_log2(n_read ? n_read : 1))
    return ppk_fail(PPK_ERR_ARG, who + ": shift must be at most 62 - ceil_log2(rows read), or a sum could pass 2^62");
  if (!finite_pos(h) || !finite_pos(h * h) || !finite_pos(1.0 / (h * h)))
    return ppk_fail(PPK_ERR_ARG, who + ": h = " + num(h) + " must be finite and positive (and h * h, 1 / (h * h) too)");
  if (scale) {
    for (int c = 0; c < 2; ++c)
      if (!finite_pos(scale[c]))
        return ppk_fail(PPK_ERR_ARG, who + ": scale[" + std::to_string(c) + "] = " + num(scale[c]) + " must be finite and positive");
  } else if (n_read == 0) {
    return ppk_fail(PPK_ERR_ARG, who + ": no rows read, so there are no column maxima: pass a scale");
  }
  int rc = kde_check_grid(who, "gx", gx, nx);
  if (rc == PPK_OK) rc = kde_check_grid(who, "gy", gy, ny);
  return rc;
}

int counts_check_args(size_t n_rows, bool has_label, int n_slots, double x0, double inv_dx, size_t nx, double y0,
                      double inv_dy, size_t ny) {
  const std::string who = kWhoCounts;
  if (n_rows >= ((size_t)1 << 32)) return ppk_fail(PPK_ERR_ARG, who + ": n_rows must be < 2^32");
  if (n_slots < 1 || n_slots > 32) return ppk_fail(PPK_ERR_ARG, who + ": n_slots must be 1 .. 32");
  if (!has_label && n_slots != 1) return ppk_fail(PPK_ERR_ARG, who + ": n_slots must be 1 without labels");
  if (nx < 1 || nx > 4096 || ny < 1 || ny > 4096) return ppk_fail(PPK_ERR_ARG, who + ": nx and ny must be 1 .. 4096");
  if ((size_t)n_slots * nx * ny > ((size_t)1 << 26)) return ppk_fail(PPK_ERR_ARG, who + ": n_slots * nx * ny must be at most 2^26");
  if (!std::isfinite(x0) || !std::isfinite(y0)) return ppk_fail(PPK_ERR_ARG, who + ": x0 and y0 must be finite");
  if (!finite_pos(inv_dx) || !finite_pos(inv_dy))
    return ppk_fail(PPK_ERR_ARG, who + ": inv_dx and inv_dy must be finite and positive");
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_density_kde_dev(const float *d_dist, size_t n_rows, const long long *d_idx, size_t n_idx,
                                   const float *scale, const double *gx, size_t nx, const double *gy, size_t ny,
                                   double h, int shift, long long *d_sum, float *scale_used, void *stream) {
  const std::string who = kWhoKde;
  const size_t n_read = d_idx ? n_idx : n_rows;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  const size_t lds_want = (size_t)PPK_DENSITY_KDE_MAX_CELLS * 8;
  const long long min_group = ppk_config().density_kde_presum.load();
  auto *kernel = min_group > 0 ? dn_kde_kernel<true> : dn_kde_kernel<false>;
  const bool big = ppk_lds_opt_in(reinterpret_cast<const void *>(kernel), dev, (int)lds_want);
  const size_t limit = (big ? lds_want : kKdeLdsDefault) / 8;
  int rc = kde_check_args(n_read, scale, gx, nx, gy, ny, h, shift, limit);
  if (rc != PPK_OK) return rc;
  if (!d_sum || (n_read && !d_dist)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  PpkCall call(dev, s);
  unsigned long long *bad;
  unsigned *keys;
  double *d_gx, *d_gy;
  rc = ppk_scratch_carve(dev, SLOT_DENSITY, [&](Carve &c) { c.take(bad, 2).take(keys, 2).take(d_gx, nx).take(d_gy, ny); });
  if (rc != PPK_OK) return rc;
  PPK_HIP(hipMemsetAsync(bad, 0xff, 16, s));
  PPK_HIP(hipMemsetAsync(d_sum, 0, nx * ny * 8, s));
  PPK_HIP(hipMemcpyAsync(d_gx, gx, nx * 8, hipMemcpyHostToDevice, s));
  PPK_HIP(hipMemcpyAsync(d_gy, gy, ny * 8, hipMemcpyHostToDevice, s));
  const unsigned cap = 2u * (unsigned)ppk_geometry(dev).cus;      // two workgroups of this LDS size to a CU
  if (scale) {
    hipLaunchKernelGGL(dn_set_scale_kernel, dim3(1), dim3(1), 0, s, keys, ord_of(scale[0]), ord_of(scale[1]));
  } else {
    PPK_HIP(hipMemsetAsync(keys, 0, 8, s));
    ppk_prof_stage("scale", s);
    hipLaunchKernelGGL(dn_scale_kernel, dim3(grid_for(n_read, (size_t)kThreads * kItems, 4 * cap)), dim3(kThreads), 0, s,
                       d_dist, n_rows, d_idx, n_read, keys);
  }
  if (n_read) {
    ppk_prof_stage("kde", s);
    const double hw = h * (1.0 + std::ldexp(1.0, -20));
    hipLaunchKernelGGL(kernel, dim3(grid_for(n_read, (size_t)kThreads * kItems, cap)), dim3(kThreads),
                       (nx * ny + nx + ny) * 8, s, d_dist, n_rows, d_idx, n_read, keys, d_gx, (int)nx, d_gy, (int)ny, hw,
                       1.0 / (h * h), std::ldexp(1.0, shift), (int)(min_group > 64 ? 64 : min_group),
                       reinterpret_cast<unsigned long long *>(d_sum), bad);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  const unsigned long long *w = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 16}, {keys, 8}}, &w)) != PPK_OK) return rc;
  if (w[0] < w[1]) {      // the first offender of the rows read, whichever kind it is
    const size_t k = (size_t)w[0];
    long long v = 0;
    PPK_HIP(hipMemcpy(&v, d_idx + k, 8, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": index " + std::to_string(k) + ": row " + std::to_string(v) + " outside [0, " +
                                     std::to_string(n_rows) + ")");
  }
  if (w[1] != ~0ull) {
    const size_t k = (size_t)w[1];
    long long r = (long long)k;
    if (d_idx) PPK_HIP(hipMemcpy(&r, d_idx + k, 8, hipMemcpyDeviceToHost));
    float xy[2] = {0.0f, 0.0f};
    PPK_HIP(hipMemcpy(xy, d_dist + 2 * (size_t)r, 8, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + (d_idx ? ": index " + std::to_string(k) : std::string()) + ": row " + std::to_string(r) +
                                     ": value (" + num(xy[0]) + ", " + num(xy[1]) + ") is not finite");
  }
  const float used[2] = {ord_inv((unsigned)(w[2] & 0xffffffffull)), ord_inv((unsigned)(w[2] >> 32))};
  for (int c = 0; c < 2; ++c)
    if (!finite_pos(used[c]))
      return ppk_fail(PPK_ERR_ARG, who + ": scale[" + std::to_string(c) + "] = " + num(used[c]) +
                                       " (the column maximum) must be finite and positive");
  if (scale_used) {
    scale_used[0] = used[0];
    scale_used[1] = used[1];
  }
  return PPK_OK;
}

extern "C" int ppk_density_kde(const float *dist, size_t n_rows, const long long *idx, size_t n_idx, const float *scale,
                               const double *gx, size_t nx, const double *gy, size_t ny, double h, int shift,
                               int device_id, long long *sum, float *scale_used) {
  if (int rc = ppk_check_device(device_id)) return rc;
  const std::string who = kWhoKde;
  const size_t n_read = idx ? n_idx : n_rows;
  // the grid before SLOT_HOST_IN is sized from it (the device call checks again, against the LDS it really gets)
  const int rc0 = kde_check_args(n_read, scale, gx, nx, gy, ny, h, shift, PPK_DENSITY_KDE_MAX_CELLS);
  if (rc0 != PPK_OK) return rc0;
  if (!sum || (n_rows && !dist)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  float *d_dist;
  long long *d_idx, *d_sum;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_dist, 2 * n_rows).take(d_idx, idx ? n_idx : 0).take(d_sum, nx * ny);
  }, [&]() -> int {
    if (n_rows) PPK_HIP(hipMemcpy(d_dist, dist, n_rows * 8, hipMemcpyHostToDevice));
    if (idx && n_idx) PPK_HIP(hipMemcpy(d_idx, idx, n_idx * 8, hipMemcpyHostToDevice));
    const int rc = ppk_density_kde_dev(d_dist, n_rows, idx ? d_idx : nullptr, n_idx, scale, gx, nx, gy, ny, h, shift,
                                       d_sum, scale_used, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(sum, d_sum, nx * ny * 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" int ppk_density_counts_dev(const float *d_dist, size_t n_rows, const int32_t *d_label, int label_lo,
                                      int n_slots, double x0, double inv_dx, size_t nx, double y0, double inv_dy,
                                      size_t ny, uint32_t *d_counts, long long *d_outside, void *stream) {
  const std::string who = kWhoCounts;
  int rc = counts_check_args(n_rows, d_label != nullptr, n_slots, x0, inv_dx, nx, y0, inv_dy, ny);
  if (rc != PPK_OK) return rc;
  if (!d_counts || !d_outside || (n_rows && !d_dist)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  unsigned long long *bad;
  rc = ppk_scratch_carve(dev, SLOT_DENSITY, [&](Carve &c) { c.take(bad, 2); });
  if (rc != PPK_OK) return rc;
  PPK_HIP(hipMemsetAsync(bad, 0xff, 16, s));
  PPK_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_slots * nx * ny * 4, s));
  PPK_HIP(hipMemsetAsync(d_outside, 0, 8, s));
  ppk_prof_stage("counts", s);
  if (n_rows) {
    const dim3 grid(grid_for(n_rows, (size_t)kThreads * kItems, 8u * (unsigned)ppk_geometry(dev).cus));
    auto *kernel = ppk_config().density_hot_table.load() ? dn_counts_kernel<true> : dn_counts_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, s, d_dist, n_rows, d_label, label_lo, n_slots, x0, inv_dx, (int)nx,
                       y0, inv_dy, (int)ny, d_counts, reinterpret_cast<unsigned long long *>(d_outside), bad);
  }
  ppk_prof_stage(nullptr, s);
  PPK_HIP(hipGetLastError());
  const unsigned long long *w = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 16}}, &w)) != PPK_OK) return rc;
  if (w[0] != ~0ull) {
    const size_t k = (size_t)w[0];
    float xy[2] = {0.0f, 0.0f};
    PPK_HIP(hipMemcpy(xy, d_dist + 2 * k, 8, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": row " + std::to_string(k) + ": value (" + num(xy[0]) + ", " + num(xy[1]) +
                                     ") is not finite");
  }
  if (w[1] != ~0ull) {
    const size_t k = (size_t)w[1];
    int32_t l = 0;
    PPK_HIP(hipMemcpy(&l, d_label + k, 4, hipMemcpyDeviceToHost));
    return ppk_fail(PPK_ERR_ARG, who + ": row " + std::to_string(k) + ": label " + std::to_string(l) + " outside [" +
                                     std::to_string(label_lo) + ", " + std::to_string((long long)label_lo + n_slots) + ")");
  }
  return PPK_OK;
}

extern "C" int ppk_density_counts(const float *dist, size_t n_rows, const int32_t *label, int label_lo, int n_slots,
                                  double x0, double inv_dx, size_t nx, double y0, double inv_dy, size_t ny, int device_id,
                                  uint32_t *counts, long long *outside) {
  const std::string who = kWhoCounts;
  const int rc0 = counts_check_args(n_rows, label != nullptr, n_slots, x0, inv_dx, nx, y0, inv_dy, ny);
  if (rc0 != PPK_OK) return rc0;
  if (!counts || !outside || (n_rows && !dist)) return ppk_fail(PPK_ERR_ARG, who + ": NULL array");
  const size_t cells = (size_t)n_slots * nx * ny;
  float *d_dist;
  int32_t *d_label;
  uint32_t *d_counts;
  long long *d_outside;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_dist, 2 * n_rows).take(d_label, label ? n_rows : 0).take(d_counts, cells).take(d_outside, 1);
  }, [&]() -> int {
    if (n_rows) PPK_HIP(hipMemcpy(d_dist, dist, n_rows * 8, hipMemcpyHostToDevice));
    if (label && n_rows) PPK_HIP(hipMemcpy(d_label, label, n_rows * 4, hipMemcpyHostToDevice));
    const int rc = ppk_density_counts_dev(d_dist, n_rows, label ? d_label : nullptr, label_lo, n_slots, x0, inv_dx, nx,
                                          y0, inv_dy, ny, d_counts, d_outside, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(counts, d_counts, cells * 4, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(outside, d_outside, 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// Assignment with a fitted BGMM model on gfx950: BGMMFit.assign -> assign_samples -> log_likelihood
// (PopPUNK/models.py:411-465, :138-192; PopPUNK/bgmm.py:100-176) on every row of a resident distance matrix, and the
// edge-list predicate of construct_network_from_assignments -> generateTuples (PopPUNK/network.py:1170-1184).
//
//  - ppk_bgmm_prepare          : the per-component constants, in double on the host (Cholesky factor with the
//                                reference's 1e-7 fallback, log-determinant, log weight)
//  - bgmm_assign_kernel        : labels (no transcendental) and / or the float32 responsibilities (fp64 exp / log)
//  - the edge predicate: ppk_boundary.hip's mask passes with BgmmPred (label == within_label) as their row predicate
//
// The per-row statement is ppk_bgmm_label / ppk_bgmm_lpr (ppk_device.h), which kernel 1's fused MODE_BGMM epilogue
// calls too.  8 B in and 4 B out per row for labels, but the pass is VALU-issue bound, not HBM bound: two IEEE float32
// divisions per row and six fp64 fused multiply-adds plus a compare-select per component (profiles/bgmm/README.md).
#include <cmath>
#include <cstring>
#include <string>

#include "ppk_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kBlock = 256;

// logsumexp over the components (scipy.special.logsumexp as bgmm.py:124 calls it: max + log sum exp(lpr - max)),
// then resp_c = exp(lpr_c - logprob) (models.py:179); lpr is re-evaluated per pass instead of being held in an
// array the compiler would have to index at run time
__device__ __forceinline__ void bgmm_resp_row(double xs, double ys, const ppk_bgmm &m, float *__restrict__ out) {
  double mx = ppk_bgmm_lpr(xs, ys, m, 0);
  for (int c = 1; c < m.K; ++c) mx = fmax(mx, ppk_bgmm_lpr(xs, ys, m, c));
  double sum = 0.0;
  for (int c = 0; c < m.K; ++c) sum += exp(ppk_bgmm_lpr(xs, ys, m, c) - mx);
  const double logprob = log(sum) + mx;
  for (int c = 0; c < m.K; ++c) out[c] = (float)exp(ppk_bgmm_lpr(xs, ys, m, c) - logprob);
}

// Two rows per lane and kBatch row pairs per lane in flight (16-byte loads when ALIGNED, else two 8-byte loads);
// labels int32 [n], resp float [n][K].  KT > 0: K as a compile-time constant (ppk_bgmm_label_k).
constexpr int kBatch = 4;
template <bool ALIGNED, int KT>
__global__ void __launch_bounds__(kBlock)
bgmm_assign_kernel(const float *__restrict__ dist, size_t n_rows, const ppk_bgmm m, int32_t *__restrict__ labels,
                   float *__restrict__ resp) {
  const size_t n_pairs = (n_rows + 1) / 2;
  const size_t step = (size_t)gridDim.x * kBlock * kBatch;
  for (size_t p0 = (size_t)blockIdx.x * kBlock * kBatch + threadIdx.x; p0 < n_pairs; p0 += step) {
    f32x4 d[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const size_t p = p0 + (size_t)j * kBlock, row = 2 * p;
      d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ALIGNED && row + 1 < n_rows) {
        d[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(dist) + p);
      } else if (row < n_rows) {
        const float2 a = reinterpret_cast<const float2 *>(dist)[row];
        d[j].x = a.x;
        d[j].y = a.y;
        if (row + 1 < n_rows) {
          const float2 b = reinterpret_cast<const float2 *>(dist)[row + 1];
          d[j].z = b.x;
          d[j].w = b.y;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const size_t row = 2 * (p0 + (size_t)j * kBlock);
      if (row >= n_rows) break;
      const bool two = row + 1 < n_rows;
      double x0, y0, x1, y1;
      ppk_bgmm_scaled(d[j].x, d[j].y, m, x0, y0);
      ppk_bgmm_scaled(d[j].z, d[j].w, m, x1, y1);
      if (labels) {
        const int l0 = ppk_bgmm_label_k<KT>(x0, y0, m), l1 = ppk_bgmm_label_k<KT>(x1, y1, m);
        if (ALIGNED && two) {
          *reinterpret_cast<int2 *>(labels + row) = make_int2(l0, l1);
        } else {
          labels[row] = l0;
          if (two) labels[row + 1] = l1;
        }
      }
      if (resp) {
        bgmm_resp_row(x0, y0, m, resp + row * (size_t)m.K);
        if (two) bgmm_resp_row(x1, y1, m, resp + (row + 1) * (size_t)m.K);
      }
    }
  }
}

// writes the model into its device slot: a kernel argument is captured at launch, so the copy is ordered on the
// stream and the caller's struct may go at once
__global__ void bgmm_store_kernel(const ppk_bgmm m, ppk_bgmm *__restrict__ dst) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(&m);
  uint32_t *d = reinterpret_cast<uint32_t *>(dst);
  for (size_t i = threadIdx.x; i < sizeof(ppk_bgmm) / 4; i += blockDim.x) d[i] = src[i];
}

}  // namespace

static_assert(sizeof(ppk_bgmm) % 8 == 0, "ppk_bgmm is copied as dwords");

template <int KT>
static void launch_assign(bool aligned, unsigned grid, const float *d_dist, size_t n_rows, const ppk_bgmm &m,
                          int32_t *d_labels, float *d_resp, hipStream_t s) {
  if (aligned)
    hipLaunchKernelGGL((bgmm_assign_kernel<true, KT>), dim3(grid), dim3(kBlock), 0, s, d_dist, n_rows, m, d_labels, d_resp);
  else
    hipLaunchKernelGGL((bgmm_assign_kernel<false, KT>), dim3(grid), dim3(kBlock), 0, s, d_dist, n_rows, m, d_labels, d_resp);
}

int ppk_launch_bgmm_assign(const float *d_dist, size_t n_rows, const ppk_bgmm &m, int32_t *d_labels, float *d_resp,
                           hipStream_t s) {
  if (n_rows == 0) return PPK_OK;
  const size_t n_pairs = (n_rows + 1) / 2;
  const unsigned grid = grid_for(n_pairs, kBlock * kBatch, 2048);
  const bool aligned = (reinterpret_cast<uintptr_t>(d_dist) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_labels) & 7) == 0;
  switch (m.K) {      // K = 2, 3, 4 with the component loop unrolled (every default PopPUNK fit: --K 2)
    case 2: launch_assign<2>(aligned, grid, d_dist, n_rows, m, d_labels, d_resp, s); break;
    case 3: launch_assign<3>(aligned, grid, d_dist, n_rows, m, d_labels, d_resp, s); break;
    case 4: launch_assign<4>(aligned, grid, d_dist, n_rows, m, d_labels, d_resp, s); break;
    default: launch_assign<0>(aligned, grid, d_dist, n_rows, m, d_labels, d_resp, s); break;
  }
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

int ppk_bgmm_to_device(int dev, const ppk_bgmm &m, const ppk_bgmm **d_model, hipStream_t s) {
  void *p = nullptr;
  int rc = ppk_scratch_get(dev, SLOT_BGMM, sizeof(ppk_bgmm), &p);
  if (rc != PPK_OK) return rc;
  hipLaunchKernelGGL(bgmm_store_kernel, dim3(1), dim3(256), 0, s, m, static_cast<ppk_bgmm *>(p));
  PPK_HIP(hipGetLastError());
  *d_model = static_cast<const ppk_bgmm *>(p);
  return PPK_OK;
}

// ---- host preparation (no device) ------------------------------------------------------------------------------
// log_multivariate_normal_density (bgmm.py:131-176): scipy.linalg.cholesky(cv, lower=True); on LinAlgError the same
// of cv + 1e-7 I; on a second failure ValueError (chol2).

extern "C" int ppk_bgmm_prepare(int K, const double *weights, const double *means, const double *covariances,
                                const double *scale, int scale_is_f64, int within_label, ppk_bgmm *out) {
  if (!weights || !means || !covariances || !scale || !out) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_prepare: NULL argument");
  if (K < 1 || K > PPK_BGMM_MAX_K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_prepare: K = " + std::to_string(K) + " is outside [1, " +
                                     std::to_string(PPK_BGMM_MAX_K) + "]");
  if (within_label < 0 || within_label >= K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_prepare: within_label " + std::to_string(within_label) + " is not a component");
  ppk_bgmm m;
  std::memset(&m, 0, sizeof(m));
  m.K = K;
  m.within_label = within_label;
  m.scale_is_f64 = scale_is_f64 ? 1 : 0;
  for (int i = 0; i < 2; ++i) {
    if (!(scale[i] > 0.0) || !std::isfinite(scale[i])) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_prepare: scale must be positive");
    m.scale_f64[i] = scale[i];
    m.scale_f32[i] = (float)scale[i];
  }
  const double log2pi = std::log(2.0 * M_PI);
  for (int c = 0; c < K; ++c) {
    const double *cv = covariances + 4 * c;
    // the reference factors the matrix as stored: LAPACK dpotrf (lower) reads the lower triangle
    double L[3];
    if (!chol2(cv[0], cv[2], cv[3], L)) {
      if (!chol2(cv[0] + 1e-7, cv[2], cv[3] + 1e-7, L))
        return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_prepare: covariance of component " + std::to_string(c) +
                                         " is not symmetric positive-definite, even with 1e-7 added to its diagonal "
                                         "('covars' must be symmetric, positive-definite)");
      m.jitter[c] = 1;
      ++m.n_jitter;
    }
    m.mean[c][0] = means[2 * c];
    m.mean[c][1] = means[2 * c + 1];
    m.chol[c][0] = L[0];
    m.chol[c][1] = L[1];
    m.chol[c][2] = L[2];
    m.inv_diag[c][0] = 1.0 / L[0];
    m.inv_diag[c][1] = 1.0 / L[2];
    ppk_lin_of(m.mean[c], L, m.inv_diag[c][0], m.inv_diag[c][1], m.lin[c]);
    const double log_det = 2.0 * (std::log(L[0]) + std::log(L[2]));
    m.log_const[c] = std::log(weights[c]) - 0.5 * (2.0 * log2pi + log_det);
  }
  *out = m;
  return PPK_OK;
}

// ---- host arrays --------------------------------------------------------------------------------------------------
// BGMMFit.assign(X) of the Python mirror: the rows go through one chunk's buffers in SLOT_HOST_IN, 8 Mi rows (64 MB
// in) at a time, each chunk uploaded, assigned and fetched in turn on the device's default stream.
extern "C" int ppk_bgmm_assign(const float *dist, size_t n_rows, const ppk_bgmm *model, int device_id, int32_t *labels,
                               float *resp) {
  if (int rc = ppk_check_device(device_id)) return rc;
  if (!model) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_assign: model is NULL");
  if (model->K < 1 || model->K > PPK_BGMM_MAX_K || model->within_label < 0 || model->within_label >= model->K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_assign: the model is not prepared (ppk_bgmm_prepare)");
  if (n_rows == 0) return PPK_OK;
  if (!dist || (!labels && !resp)) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_assign: NULL input / no output");
  if (int rc = ppk_check_arch(device_id)) return rc;
  const size_t chunk = (size_t)8 << 20;
  const size_t buf_rows = n_rows < chunk ? n_rows : chunk;
  const size_t K = (size_t)model->K;
  float *d_in, *d_resp;
  int32_t *d_lab;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_in, buf_rows * 2).take(d_lab, labels ? buf_rows : 0).take(d_resp, resp ? buf_rows * K : 0);
  }, [&]() -> int {
    // an output not asked for has no room in the layout: the kernel is told so by a null pointer
    if (!labels) d_lab = nullptr;
    if (!resp) d_resp = nullptr;
    int rc = PPK_OK;
    for (size_t r0 = 0; r0 < n_rows && rc == PPK_OK; r0 += chunk) {
      const size_t rows = n_rows - r0 < chunk ? n_rows - r0 : chunk;
      if (hipMemcpy(d_in, dist + 2 * r0, rows * 8, hipMemcpyHostToDevice) != hipSuccess) {
        rc = ppk_fail(PPK_ERR_HIP, "hipMemcpy H2D failed");
        break;
      }
      rc = ppk_launch_bgmm_assign(d_in, rows, *model, d_lab, d_resp, nullptr);
      if (rc != PPK_OK) break;
      if ((d_lab && hipMemcpy(labels + r0, d_lab, rows * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
          (d_resp && hipMemcpy(resp + r0 * K, d_resp, rows * K * 4, hipMemcpyDeviceToHost) != hipSuccess))
        rc = ppk_fail(PPK_ERR_HIP, "BGMM assignment failed on the device");
    }
    return rc;
  });
}

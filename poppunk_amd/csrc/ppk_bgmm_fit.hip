// Fitting PopPUNK's default model on gfx950: the variational Bayesian Gaussian mixture of fit2dMultiGaussian
// (PopPUNK/bgmm.py:20-45; the definition is written out in include/ppk.h, section "BGMM fit").
//
//  - bgmm_stats_kernel<MODE> : ONE streaming pass over the training rows (a resident [n][2] float32 matrix, or the rows
//                              an int64 index list names): per row the responsibilities r_k -- MODE_EM: from the K
//                              weighted log-probabilities in fp64 (the lin / log_const form of ppk_bgmm_lpr) and their
//                              log-sum-exp; MODE_LABEL: the one-hot image of a given label; MODE_NEAREST: of the nearest
//                              centre (the k-means pass, which also writes the label and counts the changed ones) -- and
//                              per component the seven sums  S r, S r d, S r d d^T (3), S r log r,  d = xs - pivot_k
//  - bgmm_final_kernel       : the per-workgroup partial sums added in a fixed order
//  - bgmm_check_kernel       : the first index outside the matrix, non-finite row and label outside [0, K)
//  - ppk_bgmm_mstep          : the M-step and the lower bound in double on the host (no device)
//
// Reduction: lane (registers, kChunk components at a time: 28 fp64 accumulators) -> wave (shuffles) -> workgroup (LDS)
// -> one partial per workgroup in global memory -> bgmm_final_kernel.  The grid is a function of the row count only and
// there is no floating-point atomic, so the same rows give the same bits on every call.  Components beyond the first
// kChunk take another sweep over the rows inside the same launch (K <= 4, every PopPUNK default, is one sweep).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / PPK_LANES;
constexpr int kChunk = 4;                 // components whose sums a lane holds in registers at a time
constexpr int kStats = PPK_BGMM_FIT_STATS;   // per component: S r, S r dx, S r dy, S r dx dx, S r dx dy, S r dy dy, S r log r
constexpr int kRowsPerThread = 8;         // sizes the grid (with kMaxGrid): a function of the row count only
constexpr unsigned kMaxGrid = 1024;
constexpr int kKmeansMaxIter = PPK_BGMM_KMEANS_MAX_ITER;

enum { MODE_EM = 0, MODE_LABEL = 1, MODE_NEAREST = 2 };

struct FitArgs {
  int K;
  float scale[2];
  double lin[PPK_BGMM_MAX_K][5];       // MODE_EM: ppk_bgmm::lin of the variational state
  double log_const[PPK_BGMM_MAX_K];    // MODE_EM: everything of the weighted log-probability that is not the quadratic form
  double pivot[PPK_BGMM_MAX_K][2];     // the moments are taken about it; MODE_NEAREST: the centres
};


// rows float2 [n_rows]; index int64 [n] or null (then n == n_rows and row i is training row i).  An index outside
// [0, n_rows) contributes nothing and is never dereferenced (bgmm_check_kernel reports it to the fit).
// labels int32 [n]: MODE_LABEL read, MODE_NEAREST read and written.  partials double [gridDim.x][K][kStats].
template <int MODE>
__global__ void __launch_bounds__(kBlock)
bgmm_stats_kernel(const float2 *__restrict__ rows, size_t n_rows, const long long *__restrict__ index, size_t n,
                  const FitArgs a, int32_t *__restrict__ labels, double *__restrict__ partials,
                  unsigned *__restrict__ n_changed) {
  __shared__ double red[kWaves][kChunk * kStats];
  const int lane = threadIdx.x & (PPK_LANES - 1), wave = threadIdx.x / PPK_LANES;
  const size_t step = (size_t)gridDim.x * kBlock;
  for (int c0 = 0; c0 < a.K; c0 += kChunk) {
    double acc[kChunk][kStats];
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
#pragma unroll
      for (int s = 0; s < kStats; ++s) acc[j][s] = 0.0;
    unsigned changed = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
      size_t row = i;
      if (index) {
        const long long r = index[i];
        if (r < 0 || (unsigned long long)r >= n_rows) continue;
        row = (size_t)r;
      }
      const float2 v = rows[row];
      const double xs = ppk_scaled_f32(v.x, a.scale[0]), ys = ppk_scaled_f32(v.y, a.scale[1]);
      double r[kChunk], rl[kChunk];
      if (MODE == MODE_EM) {
        // scipy's logsumexp: max + log sum exp(w - max); log_resp = w - that; resp = exp(log_resp)
        double mx = ppk_bgmm_lpr(xs, ys, a, 0);
        for (int c = 1; c < a.K; ++c) mx = fmax(mx, ppk_bgmm_lpr(xs, ys, a, c));
        double sum = 0.0;
        for (int c = 0; c < a.K; ++c) sum += exp(ppk_bgmm_lpr(xs, ys, a, c) - mx);
        const double lse = mx + log(sum);
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          r[j] = rl[j] = 0.0;
          if (c0 + j < a.K) {
            const double lr = ppk_bgmm_lpr(xs, ys, a, c0 + j) - lse;
            r[j] = exp(lr);
            rl[j] = r[j] * lr;
          }
        }
      } else {
        int lab;
        if (MODE == MODE_LABEL || c0 > 0) {
          lab = labels[i];                  // (MODE_NEAREST, later sweeps: what this thread wrote in the first)
        } else {
          // nearest centre under (d2, index of centre): IEEE double, nothing fused
          double best = 0.0;
          lab = 0;
          for (int c = 0; c < a.K; ++c) {
            const double dx = xs - a.pivot[c][0], dy = ys - a.pivot[c][1];
            const double d2 = dx * dx + dy * dy;
            if (c == 0 || d2 < best) {
              best = d2;
              lab = c;
            }
          }
          if (labels[i] != lab) ++changed;
          labels[i] = lab;
        }
#pragma unroll
        for (int j = 0; j < kChunk; ++j) {
          r[j] = lab == c0 + j ? 1.0 : 0.0;
          rl[j] = 0.0;
        }
      }
#pragma unroll
      for (int j = 0; j < kChunk; ++j) {
        const double dx = xs - a.pivot[c0 + j][0], dy = ys - a.pivot[c0 + j][1];
        const double rx = r[j] * dx, ry = r[j] * dy;
        acc[j][0] += r[j];
        acc[j][1] += rx;
        acc[j][2] += ry;
        acc[j][3] += rx * dx;
        acc[j][4] += rx * dy;
        acc[j][5] += ry * dy;
        acc[j][6] += rl[j];
      }
    }
    // lane -> wave -> workgroup, every step in a fixed order
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
#pragma unroll
      for (int s = 0; s < kStats; ++s) {
        const double w = wave_sum(acc[j][s], warpSize);
        if (lane == 0) red[wave][j * kStats + s] = w;
      }
    if (MODE == MODE_NEAREST && c0 == 0) {
      unsigned ch = changed;
#pragma unroll
      for (int off = PPK_LANES / 2; off > 0; off >>= 1) ch += __shfl_down(ch, off);
      if (lane == 0 && ch) atomicAdd(n_changed, ch);      // an integer count: the order of the additions is immaterial
    }
    __syncthreads();
    if (threadIdx.x < kChunk * kStats && c0 + (int)threadIdx.x / kStats < a.K) {
      double t = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t += red[w][threadIdx.x];
      partials[((size_t)blockIdx.x * a.K + c0) * kStats + threadIdx.x] = t;
    }
    __syncthreads();
  }
}

// stats[v] = the sum over the workgroups' partials[g][v]: thread t adds g = t, t + 256, ... in order, then a fixed tree
__global__ void __launch_bounds__(kBlock)
bgmm_final_kernel(const double *__restrict__ partials, unsigned n_groups, unsigned n_values, double *__restrict__ stats) {
  __shared__ double red[kBlock];
  const unsigned v = blockIdx.x;
  double t = 0.0;
  for (unsigned g = threadIdx.x; g < n_groups; g += kBlock) t += partials[(size_t)g * n_values + v];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int half = kBlock / 2; half > 0; half >>= 1) {
    if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[v] = red[0];
}

// bad[0..2] (all ones when there is none): the first position whose index is outside the matrix, whose row is not
// finite, whose label is outside [0, K)
__global__ void __launch_bounds__(kBlock)
bgmm_check_kernel(const float2 *__restrict__ rows, size_t n_rows, const long long *__restrict__ index, size_t n,
                  const int32_t *__restrict__ labels, int K, unsigned long long *__restrict__ bad) {
  const size_t step = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
    size_t row = i;
    if (index) {
      const long long r = index[i];
      if (r < 0 || (unsigned long long)r >= n_rows) {
        atomicMin(&bad[0], (unsigned long long)i);
        continue;
      }
      row = (size_t)r;
    }
    const float2 v = rows[row];
    if (!(isfinite(v.x) && isfinite(v.y))) atomicMin(&bad[1], (unsigned long long)i);
    if (labels && (labels[i] < 0 || labels[i] >= K)) atomicMin(&bad[2], (unsigned long long)i);
  }
}

unsigned stats_grid(size_t n) { return grid_for(n, (size_t)kBlock * kRowsPerThread, kMaxGrid); }

// one pass: partials, then d_stats double [K][kStats]
int launch_stats(int mode, const float *d_rows, size_t n_rows, const long long *d_index, size_t n, const FitArgs &a,
                 int32_t *d_labels, double *d_partials, unsigned *d_changed, double *d_stats, hipStream_t s) {
  const unsigned grid = stats_grid(n);
  const float2 *rows = reinterpret_cast<const float2 *>(d_rows);
  switch (mode) {
    case MODE_EM:
      hipLaunchKernelGGL(bgmm_stats_kernel<MODE_EM>, dim3(grid), dim3(kBlock), 0, s, rows, n_rows, d_index, n, a, d_labels,
                         d_partials, d_changed);
      break;
    case MODE_LABEL:
      hipLaunchKernelGGL(bgmm_stats_kernel<MODE_LABEL>, dim3(grid), dim3(kBlock), 0, s, rows, n_rows, d_index, n, a,
                         d_labels, d_partials, d_changed);
      break;
    default:
      hipLaunchKernelGGL(bgmm_stats_kernel<MODE_NEAREST>, dim3(grid), dim3(kBlock), 0, s, rows, n_rows, d_index, n, a,
                         d_labels, d_partials, d_changed);
      break;
  }
  PPK_HIP(hipGetLastError());
  hipLaunchKernelGGL(bgmm_final_kernel, dim3((unsigned)(a.K * kStats)), dim3(kBlock), 0, s, d_partials, grid,
                     (unsigned)(a.K * kStats), d_stats);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

// ---- host arithmetic ----------------------------------------------------------------------------------------------
// digamma for x > 0: psi(x) = psi(x + 1) - 1 / x up to x >= 10, then the asymptotic series
// ln x - 1/(2x) - sum B_2k / (2k x^2k) through x^-14 (its next term is below 1e-17 of psi at x = 10)
double digamma_pos(double x) {
  double shift = 0.0;
  while (x < 10.0) {
    shift -= 1.0 / x;
    x += 1.0;
  }
  const double y = 1.0 / (x * x);
  const double series = y * (1.0 / 12 - y * (1.0 / 120 - y * (1.0 / 252 - y * (1.0 / 240 - y * (1.0 / 132 - y * (691.0 / 32760 - y * (1.0 / 12)))))));
  return shift + (std::log(x) - 0.5 / x - series);
}

int check_params(const ppk_bgmm_fit_params *p, const char *who) {
  if (!p) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": params is NULL");
  if (p->K < 1 || p->K > PPK_BGMM_MAX_K)
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": K = " + std::to_string(p->K) + " is outside [1, " +
                                     std::to_string(PPK_BGMM_MAX_K) + "]");
  if (!(p->weight_concentration_prior > 0.0) || !(p->mean_precision_prior > 0.0) || !std::isfinite(p->mean_prior[0]) ||
      !std::isfinite(p->mean_prior[1]) || !(p->reg_covar >= 0.0) || !(p->tol >= 0.0))
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": the priors must be positive and finite, reg_covar and tol non-negative");
  if (!(p->degrees_of_freedom_prior > 1.0))
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": degrees_of_freedom_prior must be greater than 1 (the dimension less one)");
  if (p->max_iter < 0 || p->max_iter > PPK_BGMM_FIT_MAX_ITER)
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": max_iter = " + std::to_string(p->max_iter) + " is outside [0, " +
                                     std::to_string(PPK_BGMM_FIT_MAX_ITER) + "]");
  if (p->n_init < 1 || p->n_init > PPK_BGMM_FIT_MAX_INIT)
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": n_init = " + std::to_string(p->n_init) + " is outside [1, " +
                                     std::to_string(PPK_BGMM_FIT_MAX_INIT) + "]");
  return PPK_OK;
}

// the M-step and the bound (include/ppk.h "BGMM fit", steps M1-M5 and B)
int mstep(const ppk_bgmm_fit_params &p, const double *st, const double *pivot, const double *W0, ppk_bgmm_state *S,
          double *lower_bound) {
  const int K = p.K;
  const double eps10 = 10.0 * DBL_EPSILON, m0x = p.mean_prior[0], m0y = p.mean_prior[1];
  std::memset(S, 0, sizeof(*S));
  S->K = K;
  double nk[PPK_BGMM_MAX_K], rlogr = 0.0;
  for (int k = 0; k < K; ++k) {
    const double *t = st + (size_t)k * kStats;
    for (int s = 0; s < kStats; ++s)
      if (!std::isfinite(t[s]))
        return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_mstep: a statistic of component " + std::to_string(k) + " is not finite");
    nk[k] = t[0] + eps10;
    // one-pass moments about the pivot: xk = pivot + m, sk = S r d d^T / nk - m m^T (2 - S r / nk), m = S r d / nk,
    // which is S r (x - xk)(x - xk)^T / nk exactly; with no responsibility at all xk is 0 / nk = 0
    const double mx = t[1] / nk[k], my = t[2] / nk[k], f = 2.0 - t[0] / nk[k];
    const double xkx = t[0] == 0.0 ? 0.0 : pivot[2 * k] + mx, xky = t[0] == 0.0 ? 0.0 : pivot[2 * k + 1] + my;
    const double sxx = t[3] / nk[k] - mx * mx * f + p.reg_covar, sxy = t[4] / nk[k] - mx * my * f,
                 syy = t[5] / nk[k] - my * my * f + p.reg_covar;
    rlogr += t[6];
    S->mean_precision[k] = p.mean_precision_prior + nk[k];
    S->means[k][0] = (p.mean_precision_prior * m0x + nk[k] * xkx) / S->mean_precision[k];
    S->means[k][1] = (p.mean_precision_prior * m0y + nk[k] * xky) / S->mean_precision[k];
    S->dof[k] = p.degrees_of_freedom_prior + nk[k];
    const double dx = xkx - m0x, dy = xky - m0y, g = p.mean_precision_prior / S->mean_precision[k];
    S->covariances[k][0] = (W0[0] + nk[k] * (sxx + g * (dx * dx))) / S->dof[k];
    S->covariances[k][1] = (W0[1] + nk[k] * (sxy + g * (dx * dy))) / S->dof[k];
    S->covariances[k][2] = (W0[2] + nk[k] * (sxy + g * (dy * dx))) / S->dof[k];
    S->covariances[k][3] = (W0[3] + nk[k] * (syy + g * (dy * dy))) / S->dof[k];
    if (!chol2(S->covariances[k][0], S->covariances[k][2], S->covariances[k][3], S->chol[k]))
      return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_mstep: the covariance of component " + std::to_string(k) +
                                       " lost positive-definiteness (fitting the mixture model failed because some "
                                       "components have ill-defined empirical covariance: decrease the number of "
                                       "components or increase reg_covar)");
  }
  // Dirichlet process: a = 1 + nk, b = prior + the responsibility behind k, added from the last component down
  double tail = 0.0;
  for (int k = K - 1; k >= 0; --k) {
    S->weight_conc_a[k] = 1.0 + nk[k];
    S->weight_conc_b[k] = p.weight_concentration_prior + (k == K - 1 ? 0.0 : tail + nk[k + 1]);
    if (k < K - 1) tail += nk[k + 1];
  }
  // stick-breaking weights, and E[log w]
  double wsum = 0.0, stick = 1.0, cum = 0.0, bound_w = 0.0, bound_l = 0.0, bound_m = 0.0;
  const double log2pi = std::log(2.0 * M_PI), log2 = std::log(2.0);
  for (int k = 0; k < K; ++k) {
    const double a = S->weight_conc_a[k], b = S->weight_conc_b[k], ab = a + b;
    S->weights[k] = a / ab * stick;
    stick *= b / ab;
    wsum += S->weights[k];
    const double dsum = digamma_pos(ab);
    const double elogw = digamma_pos(a) - dsum + cum;
    cum += digamma_pos(b) - dsum;
    const double *L = S->chol[k];
    const double i0 = 1.0 / L[0], i1 = 1.0 / L[2];
    ppk_lin_of(S->means[k], L, i0, i1, S->lin[k]);
    const double dof = S->dof[k];
    const double log_det = std::log(i0) + std::log(i1);                 // of the precision's Cholesky factor
    const double log_lambda = 2.0 * log2 + digamma_pos(0.5 * dof) + digamma_pos(0.5 * (dof - 1.0));
    S->log_const[k] = (-0.5 * (2.0 * log2pi) + log_det) - 0.5 * 2.0 * std::log(dof) +
                      0.5 * (log_lambda - 2.0 / S->mean_precision[k]) + elogw;
    const double ldpc = log_det - 0.5 * 2.0 * std::log(dof);
    bound_w += -(dof * ldpc + dof * 2.0 * 0.5 * log2 + std::lgamma(0.5 * dof) + std::lgamma(0.5 * (dof - 1.0)));
    bound_l += std::lgamma(a) + std::lgamma(b) - std::lgamma(ab);    // betaln
    bound_m += std::log(S->mean_precision[k]);
  }
  for (int k = 0; k < K; ++k) S->weights[k] /= wsum;
  if (lower_bound) *lower_bound = -rlogr - bound_w + bound_l - 0.5 * 2.0 * bound_m;
  return PPK_OK;
}

void args_from_state(const ppk_bgmm_state &S, const float *scale, FitArgs *a) {
  std::memset(a, 0, sizeof(*a));
  a->K = S.K;
  a->scale[0] = scale[0];
  a->scale[1] = scale[1];
  std::memcpy(a->lin, S.lin, sizeof(a->lin));
  std::memcpy(a->log_const, S.log_const, sizeof(a->log_const));
  std::memcpy(a->pivot, S.means, sizeof(a->pivot));
}

void args_from_pivot(int K, const double *pivot, const float *scale, FitArgs *a) {
  std::memset(a, 0, sizeof(*a));
  a->K = K;
  a->scale[0] = scale[0];
  a->scale[1] = scale[1];
  for (int k = 0; k < K; ++k) {
    a->pivot[k][0] = pivot[2 * k];
    a->pivot[k][1] = pivot[2 * k + 1];
  }
}

int check_rows(const char *who, const void *d_rows, size_t n_rows, const void *d_index, size_t n_index, const float *scale,
               size_t *n_train) {
  if (!d_rows || !scale) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": NULL rows / scale");
  if (!(scale[0] > 0.0f) || !(scale[1] > 0.0f) || !std::isfinite(scale[0]) || !std::isfinite(scale[1]))
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": scale must be positive");
  if (n_rows >= ((size_t)1 << 40)) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": n_rows must be < 2^40");
  *n_train = d_index ? n_index : n_rows;
  if (*n_train >= ((size_t)1 << 40)) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": n_index must be < 2^40");
  return PPK_OK;
}

struct FitScratch {
  double *partials, *stats;
  unsigned long long *bad;
  unsigned *changed;
  int32_t *labels;
};

int carve_fit(int dev, int K, size_t n_train, bool want_labels, FitScratch *f) {
  return ppk_scratch_carve(dev, SLOT_BGMM_FIT, [&](Carve &c) {
    c.take(f->partials, (size_t)stats_grid(n_train) * K * kStats).take(f->stats, (size_t)K * kStats);
    c.take(f->bad, 4).take(f->changed, 2).take(f->labels, want_labels ? n_train : 1);
  });
}

}  // namespace

static_assert(sizeof(FitArgs) <= 2048, "FitArgs travels as a kernel argument");

extern "C" int ppk_bgmm_fit_params_default(int K, ppk_bgmm_fit_params *out) {
  if (!out) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit_params_default: NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->K = K;
  out->max_iter = 100;
  out->n_init = 5;
  out->weight_concentration_prior = 0.1;
  out->mean_precision_prior = 0.1;
  out->degrees_of_freedom_prior = 2.0;
  out->reg_covar = 1e-6;
  out->tol = 1e-3;
  return check_params(out, "ppk_bgmm_fit_params_default");
}

extern "C" int ppk_bgmm_fit_struct_sizes(size_t out[3]) {
  if (!out) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit_struct_sizes: NULL argument");
  out[0] = sizeof(ppk_bgmm_fit_params);
  out[1] = sizeof(ppk_bgmm_state);
  out[2] = sizeof(ppk_bgmm_fit_result);
  return PPK_OK;
}

extern "C" double ppk_bgmm_digamma(double x) { return x > 0.0 ? digamma_pos(x) : NAN; }

extern "C" int ppk_bgmm_mstep(const ppk_bgmm_fit_params *params, const double *stats, const double *pivot,
                              const double *cov_prior, ppk_bgmm_state *state_out, double *lower_bound_out) {
  if (int rc = check_params(params, "ppk_bgmm_mstep")) return rc;
  if (!stats || !pivot || !cov_prior || !state_out) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_mstep: NULL argument");
  return mstep(*params, stats, pivot, cov_prior, state_out, lower_bound_out);
}

extern "C" int ppk_bgmm_stats_dev(const float *d_rows, size_t n_rows, const long long *d_index, size_t n_index,
                                  const float *scale, const ppk_bgmm_state *state, double *d_stats, void *stream) {
  size_t n = 0;
  if (int rc = check_rows("ppk_bgmm_stats", d_rows, n_rows, d_index, n_index, scale, &n)) return rc;
  if (!state || !d_stats) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_stats: NULL state / output");
  if (state->K < 1 || state->K > PPK_BGMM_MAX_K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_stats: K = " + std::to_string(state->K) + " is outside [1, " +
                                     std::to_string(PPK_BGMM_MAX_K) + "]");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  FitScratch f;
  if (int rc = carve_fit(dev, state->K, n, false, &f)) return rc;
  FitArgs a;
  args_from_state(*state, scale, &a);
  return launch_stats(MODE_EM, d_rows, n_rows, d_index, n, a, nullptr, f.partials, f.changed, d_stats, s);
}

extern "C" int ppk_bgmm_kmeans_dev(const float *d_rows, size_t n_rows, const long long *d_index, size_t n_index,
                                   const float *scale, int K, const double *centres, int32_t *d_labels, double *d_stats,
                                   unsigned *d_changed, void *stream) {
  size_t n = 0;
  if (int rc = check_rows("ppk_bgmm_kmeans", d_rows, n_rows, d_index, n_index, scale, &n)) return rc;
  if (!centres || !d_labels || !d_stats || !d_changed) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_kmeans: NULL argument");
  if (K < 1 || K > PPK_BGMM_MAX_K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_kmeans: K = " + std::to_string(K) + " is outside [1, " +
                                     std::to_string(PPK_BGMM_MAX_K) + "]");
  for (int k = 0; k < 2 * K; ++k)
    if (!std::isfinite(centres[k])) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_kmeans: centre " + std::to_string(k / 2) + " is not finite");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  FitScratch f;
  if (int rc = carve_fit(dev, K, n, false, &f)) return rc;
  FitArgs a;
  args_from_pivot(K, centres, scale, &a);
  PPK_HIP(hipMemsetAsync(d_changed, 0, sizeof(unsigned), s));
  return launch_stats(MODE_NEAREST, d_rows, n_rows, d_index, n, a, d_labels, f.partials, d_changed, d_stats, s);
}

extern "C" int ppk_bgmm_fit_dev(const float *d_rows, size_t n_rows, const long long *d_index, size_t n_index,
                                const float *scale, const int32_t *d_init_labels, const double *init_centres,
                                const ppk_bgmm_fit_params *params, ppk_bgmm_fit_result *result, void *stream) {
  if (int rc = check_params(params, "ppk_bgmm_fit")) return rc;
  size_t n = 0;
  if (int rc = check_rows("ppk_bgmm_fit", d_rows, n_rows, d_index, n_index, scale, &n)) return rc;
  if (!result) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: result is NULL");
  if ((d_init_labels == nullptr) == (init_centres == nullptr))
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: give either the initial labels or the initial centres of every run");
  const ppk_bgmm_fit_params &p = *params;
  const int K = p.K;
  if (n < 2) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: fewer than 2 training rows (" + std::to_string(n) + ")");
  if (n < (size_t)K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: fewer training rows (" + std::to_string(n) + ") than components (" +
                                     std::to_string(K) + ")");
  const int n_runs = d_init_labels ? 1 : p.n_init;      // runs from the same labels would be the same run
  if (init_centres)
    for (int k = 0; k < n_runs * K * 2; ++k)
      if (!std::isfinite(init_centres[k]))
        return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: initial centre " + std::to_string((k / 2) % K) + " of run " +
                                         std::to_string(k / (2 * K)) + " is not finite");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  // whichever way the call returns, the stage that is open then is closed (closing with none open does nothing)
  struct StageEnd {
    hipStream_t s;
    ~StageEnd() { ppk_prof_stage(nullptr, s); }
  } stage_end{s};
  FitScratch f;
  if (int rc = carve_fit(dev, K, n, init_centres != nullptr, &f)) return rc;
  const unsigned long long *h = nullptr;
  const double *hs = nullptr;
  int rc;

  // -- the rows: indices inside the matrix, finite values, labels inside [0, K)
  ppk_prof_stage("bgmm_fit_check", s);
  PPK_HIP(hipMemsetAsync(f.bad, 0xff, 3 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(bgmm_check_kernel, dim3(stats_grid(n)), dim3(kBlock), 0, s, reinterpret_cast<const float2 *>(d_rows),
                     n_rows, d_index, n, d_init_labels, K, f.bad);
  PPK_HIP(hipGetLastError());
  if ((rc = ppk_read_back(dev, s, {{f.bad, 24}}, &h)) != PPK_OK) return rc;
  ppk_prof_stage(nullptr, s);
  if (h[0] != ~0ull)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: index entry " + std::to_string(h[0]) + " is outside the matrix of " +
                                     std::to_string(n_rows) + " rows");
  if (h[1] != ~0ull)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: training row " + std::to_string(h[1]) + " is not finite");
  if (h[2] != ~0ull)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: the label of training row " + std::to_string(h[2]) + " is outside [0, " +
                                     std::to_string(K) + ")");

  // -- covariance prior: np.cov of the training points, as the K = 1, r = 1 statistics about their mean
  ppk_prof_stage("bgmm_fit_prior", s);
  FitArgs a;
  double pivot[2 * PPK_BGMM_MAX_K] = {0.0, 0.0};
  double st[PPK_BGMM_MAX_K * kStats];
  for (int pass = 0; pass < 2; ++pass) {
    // one component whose log-probability is the constant 0 (lin and log_const all zero): r = exp(0 - log 1) = 1 and
    // r log r = 0 for every row, exactly; about the origin first, then about the mean that gives
    args_from_pivot(1, pivot, scale, &a);
    if ((rc = launch_stats(MODE_EM, d_rows, n_rows, d_index, n, a, nullptr, f.partials, f.changed, f.stats, s)) != PPK_OK)
      return rc;
    if ((rc = ppk_read_back(dev, s, {{f.stats, kStats * 8}}, &h)) != PPK_OK) return rc;
    hs = reinterpret_cast<const double *>(h);
    if (pass == 0) {
      pivot[0] = hs[1] / hs[0];
      pivot[1] = hs[2] / hs[0];
    }
  }
  ppk_prof_stage(nullptr, s);
  {
    const double cnt = hs[0], mx = hs[1] / cnt, my = hs[2] / cnt;
    result->cov_prior[0] = (hs[3] - cnt * mx * mx) / (cnt - 1.0);
    result->cov_prior[1] = result->cov_prior[2] = (hs[4] - cnt * mx * my) / (cnt - 1.0);
    result->cov_prior[3] = (hs[5] - cnt * my * my) / (cnt - 1.0);
    result->train_mean[0] = pivot[0] + mx;
    result->train_mean[1] = pivot[1] + my;
  }
  const double mean0[2] = {result->train_mean[0], result->train_mean[1]};
  double W0[4];
  std::memcpy(W0, result->cov_prior, sizeof(W0));

  result->n_train = n;
  result->n_init_run = n_runs;
  result->best_init = -1;
  result->n_iter = 0;
  result->converged = 0;
  result->lower_bound = -INFINITY;
  std::vector<double> trace((size_t)p.max_iter + 1);
  for (int run = 0; run < n_runs; ++run) {
    // -- labels of this run: given, or Lloyd's iterations from the run's centres
    const int32_t *labels = d_init_labels;
    result->kmeans_iter[run] = 0;
    if (!labels) {
      ppk_prof_stage("bgmm_fit_kmeans", s);
      double centres[2 * PPK_BGMM_MAX_K];
      std::memcpy(centres, init_centres + (size_t)run * 2 * K, sizeof(double) * 2 * K);
      PPK_HIP(hipMemsetAsync(f.labels, 0xff, n * sizeof(int32_t), s));
      for (int it = 1; it <= kKmeansMaxIter; ++it) {
        args_from_pivot(K, centres, scale, &a);
        PPK_HIP(hipMemsetAsync(f.changed, 0, sizeof(unsigned), s));
        if ((rc = launch_stats(MODE_NEAREST, d_rows, n_rows, d_index, n, a, f.labels, f.partials, f.changed, f.stats, s)) != PPK_OK)
          return rc;
        if ((rc = ppk_read_back(dev, s, {{f.stats, (size_t)K * kStats * 8}, {f.changed, 4}}, &h)) != PPK_OK) return rc;
        hs = reinterpret_cast<const double *>(h);
        result->kmeans_iter[run] = it;
        const unsigned changed = (unsigned)(h[(size_t)K * kStats] & 0xffffffffull);
        if (!changed) break;
        for (int k = 0; k < K; ++k)
          if (hs[k * kStats] > 0.0) {        // an emptied centre keeps its place
            centres[2 * k] += hs[k * kStats + 1] / hs[k * kStats];
            centres[2 * k + 1] += hs[k * kStats + 2] / hs[k * kStats];
          }
      }
      ppk_prof_stage(nullptr, s);
      labels = f.labels;
    }
    // -- initialisation: the statistics of the one-hot responsibilities, about the training mean first and then about
    //    the component means that gives
    ppk_prof_stage("bgmm_fit_init", s);
    for (int k = 0; k < K; ++k) {
      pivot[2 * k] = mean0[0];
      pivot[2 * k + 1] = mean0[1];
    }
    for (int pass = 0; pass < 2; ++pass) {
      args_from_pivot(K, pivot, scale, &a);
      if ((rc = launch_stats(MODE_LABEL, d_rows, n_rows, d_index, n, a, const_cast<int32_t *>(labels), f.partials, f.changed,
                             f.stats, s)) != PPK_OK)
        return rc;
      if ((rc = ppk_read_back(dev, s, {{f.stats, (size_t)K * kStats * 8}}, &h)) != PPK_OK) return rc;
      hs = reinterpret_cast<const double *>(h);
      if (pass == 0)
        for (int k = 0; k < K; ++k)
          if (hs[k * kStats] > 0.0) {
            pivot[2 * k] += hs[k * kStats + 1] / hs[k * kStats];
            pivot[2 * k + 1] += hs[k * kStats + 2] / hs[k * kStats];
          }
    }
    ppk_prof_stage(nullptr, s);
    std::memcpy(st, hs, sizeof(double) * K * kStats);
    ppk_bgmm_state S;
    if ((rc = mstep(p, st, pivot, W0, &S, nullptr)) != PPK_OK) return rc;

    // -- variational EM: one pass and one synchronisation per iteration
    ppk_prof_stage("bgmm_fit_em", s);
    double lb = -INFINITY;
    int n_iter = 0, converged = 0;
    for (int it = 1; it <= p.max_iter; ++it) {
      const double prev = lb;
      args_from_state(S, scale, &a);
      if ((rc = launch_stats(MODE_EM, d_rows, n_rows, d_index, n, a, nullptr, f.partials, f.changed, f.stats, s)) != PPK_OK)
        return rc;
      if ((rc = ppk_read_back(dev, s, {{f.stats, (size_t)K * kStats * 8}}, &h)) != PPK_OK) return rc;
      std::memcpy(st, h, sizeof(double) * K * kStats);
      for (int k = 0; k < K; ++k) {
        pivot[2 * k] = S.means[k][0];
        pivot[2 * k + 1] = S.means[k][1];
      }
      if ((rc = mstep(p, st, pivot, W0, &S, &lb)) != PPK_OK) return rc;
      trace[it - 1] = lb;
      n_iter = it;
      if (std::fabs(lb - prev) < p.tol) {
        converged = 1;
        break;
      }
    }
    ppk_prof_stage(nullptr, s);
    result->init_lower_bound[run] = lb;
    result->init_n_iter[run] = n_iter;
    // the greatest bound wins, the first on ties; a run that made no iteration has none and wins only as the first
    if (result->best_init < 0 || lb > result->lower_bound) {
      result->best_init = run;
      result->state = S;
      result->n_iter = n_iter;
      result->converged = converged;
      result->lower_bound = lb;
      std::memset(result->lower_bounds, 0, sizeof(result->lower_bounds));
      for (int i = 0; i < n_iter; ++i) result->lower_bounds[i] = trace[i];
    }
  }
  return PPK_OK;
}

extern "C" int ppk_bgmm_fit(const float *rows, size_t n_rows, const long long *index, size_t n_index, const float *scale,
                            const int32_t *init_labels, const double *init_centres, const ppk_bgmm_fit_params *params,
                            int device_id, ppk_bgmm_fit_result *result) {
  if (int rc = ppk_check_device(device_id)) return rc;
  if (int rc = check_params(params, "ppk_bgmm_fit")) return rc;
  if (!rows || !scale || !result) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: NULL rows / scale / result");
  const size_t n = index ? n_index : n_rows;
  if (index)
    for (size_t i = 0; i < n; ++i)
      if (index[i] < 0 || (unsigned long long)index[i] >= n_rows)
        return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: index entry " + std::to_string(i) + " is outside the matrix of " +
                                         std::to_string(n_rows) + " rows");
  if (n < 2) return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: fewer than 2 training rows (" + std::to_string(n) + ")");
  if (n < (size_t)params->K)
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: fewer training rows (" + std::to_string(n) + ") than components (" +
                                     std::to_string(params->K) + ")");
  if (!(scale[0] > 0.0f) || !(scale[1] > 0.0f) || !std::isfinite(scale[0]) || !std::isfinite(scale[1]))
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: scale must be positive");
  if ((init_labels == nullptr) == (init_centres == nullptr))
    return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: give either the initial labels or the initial centres of every run");
  // what the device form finds in its first pass, found here before a device is touched
  for (size_t i = 0; i < n; ++i) {
    const size_t r = index ? (size_t)index[i] : i;
    if (!std::isfinite(rows[2 * r]) || !std::isfinite(rows[2 * r + 1]))
      return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: training row " + std::to_string(i) + " is not finite");
    if (init_labels && (init_labels[i] < 0 || init_labels[i] >= params->K))
      return ppk_fail(PPK_ERR_ARG, "ppk_bgmm_fit: the label of training row " + std::to_string(i) + " is outside [0, " +
                                       std::to_string(params->K) + ")");
  }
  if (int rc = ppk_check_arch(device_id)) return rc;
  // the training rows go up gathered, in the order of the index list: the device then sees what ppk_bgmm_fit_dev
  // sees through the list, and the sums are the same bits
  float *d_in;
  int32_t *d_lab;
  return ppk_host_frame(device_id, [&](Carve &c) { c.take(d_in, 2 * n).take(d_lab, init_labels ? n : 1); }, [&]() -> int {
    if (index) {
      std::vector<float> g(2 * n);
      for (size_t i = 0; i < n; ++i) {
        g[2 * i] = rows[2 * (size_t)index[i]];
        g[2 * i + 1] = rows[2 * (size_t)index[i] + 1];
      }
      PPK_HIP(hipMemcpy(d_in, g.data(), n * 8, hipMemcpyHostToDevice));
    } else {
      PPK_HIP(hipMemcpy(d_in, rows, n * 8, hipMemcpyHostToDevice));
    }
    if (init_labels) PPK_HIP(hipMemcpy(d_lab, init_labels, n * 4, hipMemcpyHostToDevice));
    return ppk_bgmm_fit_dev(d_in, n, nullptr, 0, scale, init_labels ? d_lab : nullptr, init_centres, params, result, nullptr);
  });
}

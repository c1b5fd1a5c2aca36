// Stochastic cluster embeddings on the device: the 2-D coordinates behind the Microreact view,
// from k-nearest-neighbour lists in get_kNN_distances form.
//
//  - ppk_embed_weights_dev : lists -> P (per-row perplexity calibration) and the integer sampling weights.  Stages
//    (ppk_prof_stages names):
//      check       the lists (j in range and != i, rows grouped, distances finite and >= 0); the call's ONE
//                  synchronisation reads the first bad entry
//      calibrate   the distances' sum of squares (fixed-order partial sums), then one thread per row bisects beta
//  - ppk_embed_dev : P + lists -> Y.  Stages:
//      check       as above for the lists and P
//      weights     c = rint(P * 2^52) and its inclusive prefix; the call's ONE synchronisation reads the first bad
//                  entry and the total
//      init        Y from the generator, Eq = 1, the deltas zero
//      step        one launch per iteration: every worker draws its pairs from that iteration's snapshot of Y and
//                  adds its moves to the int64 Q32.32 deltas; q of the repulsive pairs into an int64 sum
//      apply       one launch per iteration: Y += deltas * 2^-32, the deltas back to zero, Eq folded
//    The only atomics are integer adds (and the check's integer minimum), so every run gives the same bits, and the
//    same bits as the host restatement (tests/test_embed_host.py).  No float atomics, no host round trip between
//    iterations.
#include <cmath>
#include <cstring>
#include <rocprim/device/device_scan.hpp>
#include <string>

#include "ppk_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kSumParts = 256;      // blocks of the sum of squares (a fixed count: a fixed summation order)
constexpr int kCalSteps = 256;           // bisection steps of the calibration at most
constexpr double kCalTol = 0x1p-48;      // ... which stops once hi - lo <= hi * kCalTol
constexpr long long kPoll = 256;         // iterations between two interrupt checks
constexpr double kGainClip = 0.1;        // |gain| of one pair update per coordinate at most
constexpr int kHighShift = 20;           // the weights' sum is refused once sum(c >> 20) >= 2^43: the sum of c is
constexpr unsigned long long kHighMax = 1ull << 43;   // then >= 2^63 (a sum of P of 2048), and below it < 2^63 + m 2^20
constexpr unsigned long long kGolden = 0x9E3779B97F4A7C15ull;
constexpr unsigned long long kInitKey = 0xD1B54A32D192ED03ull;

// ---- the generator (restated in tests/test_embed_host.py) ---------------------------------------------------------
// fmix = splitmix64's finaliser (ppk_device.h).  Iteration t's key is fmix(seed + (t + 1) * G); draw d of worker w in
// that iteration is fmix(key + ((w << 8 | d) + 1) * G).  Initial positions use the key fmix(seed ^ kInitKey) and the
// counter 2v + c.
__host__ __device__ __forceinline__ unsigned long long fmix(unsigned long long z) { return ppk_fmix64(z); }
__host__ __device__ __forceinline__ unsigned long long draw(unsigned long long key, unsigned long long ctr) {
  return fmix(key + (ctr + 1) * kGolden);
}
unsigned long long iter_key(unsigned long long seed, long long t) {
  return fmix(seed + (unsigned long long)(t + 1) * kGolden);
}

// Q32.32 of x: rint(x * 2^32), ties to even (x is bounded by the caller)
__device__ __forceinline__ long long fixed(double x) { return __double2ll_rn(x * 4294967296.0); }

__device__ __forceinline__ void add_fixed(long long *p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// ---- check ---------------------------------------------------------------------------------------------------------
// The first entry e of n*k that breaks a rule: i[e] == e / k, 0 <= j[e] < n, j[e] != i[e], dist[e] finite and >= 0
// (dist nullable), P[e] in [0, 1] (P nullable; NaN fails).
__global__ void __launch_bounds__(kThreads) embed_check_kernel(const long long *__restrict__ ii,
                                                               const long long *__restrict__ jj,
                                                               const float *__restrict__ dist,
                                                               const double *__restrict__ P, size_t n, size_t k,
                                                               unsigned long long *bad) {
  const size_t m = n * k;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (size_t)gridDim.x * blockDim.x) {
    const long long i = ii[e], j = jj[e];
    bool ok = i == (long long)(e / k) && j >= 0 && j < (long long)n && j != i;
    if (dist) ok = ok && isfinite(dist[e]) && dist[e] >= 0.0f;
    if (P) ok = ok && P[e] >= 0.0 && P[e] <= 1.0;
    if (!ok) atomicMin(bad, (unsigned long long)e);
  }
}

// ---- calibrate -----------------------------------------------------------------------------------------------------
__device__ void block_sum(double &v) {
  __shared__ double sh[kThreads];
  sh[threadIdx.x] = v;
  __syncthreads();
  for (unsigned h = kThreads / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
    __syncthreads();
  }
  v = sh[0];
}

// part[b] = the sum of dist^2 over the entries of block b's grid stride, in a fixed order (kSumParts blocks)
__global__ void __launch_bounds__(kThreads) embed_sumsq_kernel(const float *__restrict__ dist, size_t m,
                                                               double *part) {
  double s = 0.0;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (size_t)gridDim.x * blockDim.x) {
    const double d = (double)dist[e];
    s += d * d;
  }
  block_sum(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// rms[0] = sqrt(sum / m), or 1 when every distance is 0 (one block)
__global__ void __launch_bounds__(kThreads) embed_rms_kernel(const double *part, size_t m, double *rms) {
  double s = 0.0;
  for (unsigned b = threadIdx.x; b < kSumParts; b += kThreads) s += part[b];
  block_sum(s);
  if (threadIdx.x == 0) rms[0] = s > 0.0 ? sqrt(s / (double)m) : 1.0;
}

// One thread per row r: x_j = (dist[r, j] / rms)^2 - min_j of the same, then beta by bisection (doubling while no
// upper bound is known) until H(beta) = ln(perplexity) is bracketed within hi * kCalTol, at most kCalSteps steps.
// P[r, j] = (p_j / Z) / n with p_j = exp(-beta x_j), Z = sum p_j; c[r, j] = rint(P * 2^52).
// steps = 0 (k <= perplexity: no beta reaches the target) takes beta = 2^-256, where 256 halvings from 1 end, without
// asking H: at k == perplexity H(beta) = ln k - beta^2 Var(x) / 2 is within rounding of the target up to beta ~ 1e-8,
// and which way H > target then falls depends on the last bit of log.
__global__ void __launch_bounds__(kThreads) embed_calibrate_kernel(const float *__restrict__ dist, size_t n, size_t k,
                                                                   const double *rms_p, double target, int steps,
                                                                   double *P, unsigned long long *c) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float *row = dist + r * k;
  const double rms = rms_p[0];
  double xmin = INFINITY;
  for (size_t j = 0; j < k; ++j) {
    const double x = (double)row[j] / rms;
    xmin = fmin(xmin, x * x);
  }
  double beta = steps ? 1.0 : 0x1p-256, lo = 0.0, hi = INFINITY;
  for (int step = 0; step < steps; ++step) {
    double Z = 0.0, S = 0.0;
    for (size_t j = 0; j < k; ++j) {
      const double x = (double)row[j] / rms;
      const double x2 = x * x - xmin;
      const double p = exp(-beta * x2);
      Z += p;
      S += p * x2;
    }
    const double H = log(Z) + beta * S / Z;
    if (H > target) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = (lo + beta) / 2.0;
    }
    if (hi != INFINITY && hi - lo <= hi * kCalTol) break;
  }
  double Z = 0.0;
  for (size_t j = 0; j < k; ++j) {
    const double x = (double)row[j] / rms;
    Z += exp(-beta * (x * x - xmin));
  }
  for (size_t j = 0; j < k; ++j) {
    const double x = (double)row[j] / rms;
    const double p = exp(-beta * (x * x - xmin)) / Z / (double)n;
    P[r * k + j] = p;
    if (c) c[r * k + j] = (unsigned long long)rint(p * 0x1p52);
  }
}

// ---- weights / init ------------------------------------------------------------------------------------------------
// c = rint(P * 2^52); high[0] += sum of c >> kHighShift, one integer atomic per wave (order-free).  Every term is at
// most 2^32 (P <= 1 past the check; anything else is refused before the sum is looked at), so the high sum itself
// cannot wrap below 2^32 entries.
__global__ void __launch_bounds__(kThreads) embed_quantise_kernel(const double *__restrict__ P, size_t m,
                                                                  unsigned long long *c, unsigned long long *high) {
  unsigned long long hs = 0;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long v = (unsigned long long)rint(P[e] * 0x1p52);
    c[e] = v;
    hs += v >> kHighShift;
  }
  for (int o = PPK_LANES / 2; o > 0; o >>= 1) hs += __shfl_xor(hs, o);
  if ((threadIdx.x & (PPK_LANES - 1)) == 0 && hs) atomicAdd(high, hs);
}

// Y[v][c] = ((u53 * 2^-53) * 2 - 1) * 1e-4 from draw 2v + c of the init key; Eq = 1; the deltas and q sums zero
__global__ void __launch_bounds__(kThreads) embed_init_kernel(size_t n, unsigned long long key, double *Y,
                                                              long long *delta, long long *qacc, double *Eq) {
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < 2 * n; x += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long r = draw(key, x);
    Y[x] = (((double)(r >> 11) * 0x1p-53) * 2.0 - 1.0) * 1e-4;
    delta[x] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    qacc[0] = 0;
    qacc[1] = 0;
    Eq[0] = 1.0;
  }
}

// ---- step / apply --------------------------------------------------------------------------------------------------
// The move of one pair (a, b) from the snapshot Y: attractive g = -4q, repulsive g = 4q^2 / Eq; gain = (eta g) dY,
// clipped to +-kGainClip per coordinate, added to a and subtracted from b.  Returns q.
__device__ __forceinline__ double pair_move(const double *__restrict__ Y, long long a, long long b, bool attract,
                                            double eta, double eq, long long *delta) {
  const double dx = Y[2 * a] - Y[2 * b], dy = Y[2 * a + 1] - Y[2 * b + 1];
  const double d2 = dx * dx + dy * dy;
  const double q = 1.0 / (1.0 + d2);
  const double g = attract ? -4.0 * q : 4.0 * q * q / eq;
  const double s = eta * g;
  const long long fx = fixed(fmin(fmax(s * dx, -kGainClip), kGainClip));
  const long long fy = fixed(fmin(fmax(s * dy, -kGainClip), kGainClip));
  add_fixed(delta + 2 * a, fx);
  add_fixed(delta + 2 * a + 1, fy);
  add_fixed(delta + 2 * b, -fx);
  add_fixed(delta + 2 * b + 1, -fy);
  return q;
}

// Worker w: draw 0 picks the attractive edge upper_bound(prefix, mulhi(r, total)); draws 1 + 2s and 2 + 2s pick the
// repulsive pair (k, l) = (mulhi(r, n), mulhi(r', n)) of sample s, skipped when k == l.  Q32.32 q of the repulsive
// pairs and their count go to qacc, one atomic pair per wave.
__global__ void __launch_bounds__(kThreads) embed_step_kernel(const double *__restrict__ Y,
                                                              const unsigned long long *__restrict__ prefix, size_t m,
                                                              const long long *__restrict__ ii,
                                                              const long long *__restrict__ jj, size_t n,
                                                              unsigned long long w_count, int n_repu,
                                                              unsigned long long key, double eta, const double *Eq_p,
                                                              long long *delta, long long *qacc) {
  const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long qs = 0, qc = 0;
  if (w < w_count) {
    const double eq = Eq_p[0];
    const unsigned long long total = prefix[m - 1];
    const unsigned long long x = __umul64hi(draw(key, w << 8), total);
    size_t lo = 0, hi = m;                 // the first e with prefix[e] > x
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (prefix[mid] > x) hi = mid;
      else lo = mid + 1;
    }
    const size_t e = lo < m ? lo : m - 1;
    pair_move(Y, ii[e], jj[e], true, eta, eq, delta);
    for (int s = 0; s < n_repu; ++s) {
      const long long a = (long long)__umul64hi(draw(key, (w << 8) | (unsigned long long)(1 + 2 * s)), n);
      const long long b = (long long)__umul64hi(draw(key, (w << 8) | (unsigned long long)(2 + 2 * s)), n);
      if (a == b) continue;
      qs += fixed(pair_move(Y, a, b, false, eta, eq, delta));
      ++qc;
    }
  }
  for (int o = PPK_LANES / 2; o > 0; o >>= 1) {
    qs += __shfl_xor(qs, o);
    qc += __shfl_xor(qc, o);
  }
  if ((threadIdx.x & (PPK_LANES - 1)) == 0 && qc) {
    add_fixed(qacc, qs);
    add_fixed(qacc + 1, qc);
  }
}

// Y += delta * 2^-32 and delta = 0; thread 0 folds Eq = (Eq nsq + qsum 2^-32) / (nsq + qcount) and zeroes the sums
__global__ void __launch_bounds__(kThreads) embed_apply_kernel(double *Y, long long *delta, size_t n, double nsq,
                                                               long long *qacc, double *Eq) {
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < 2 * n; x += (size_t)gridDim.x * blockDim.x) {
    Y[x] = Y[x] + (double)delta[x] * 0x1p-32;
    delta[x] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    Eq[0] = (Eq[0] * nsq + (double)qacc[0] * 0x1p-32) / (nsq + (double)qacc[1]);
    qacc[0] = 0;
    qacc[1] = 0;
  }
}

int check_sizes(const char *who, size_t n, size_t k) {
  if (n < 2) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": n must be at least 2");
  if (n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": n must be < 2^31");
  if (k < 1 || k > n - 1)
    return ppk_fail(PPK_ERR_ARG, std::string(who) + ": k = " + std::to_string(k) + " must be in [1, n - 1]");
  return PPK_OK;
}

// the error that names bad entry e (device reads on the failure path only)
int bad_entry(const char *who, const long long *d_i, const long long *d_j, const float *d_dist, const double *d_P,
              size_t n, size_t k, size_t e) {
  long long i = 0, j = 0;
  if (!ppk_read_edge(d_i, d_j, 1, nullptr, e, &i, &j, nullptr))
    return ppk_fail(PPK_ERR_HIP, std::string(who) + ": cannot read entry " + std::to_string(e));
  std::string what;
  if (i != (long long)(e / k)) {
    what = "i = " + std::to_string(i) + " is not e / k = " + std::to_string(e / k) + " (rows grouped, k per row)";
  } else if (j < 0 || j >= (long long)n) {
    what = "j = " + std::to_string(j) + " is outside [0, " + std::to_string(n) + ")";
  } else if (j == i) {
    what = "j = i = " + std::to_string(i);
  } else {
    double v = 0.0;
    const char *name = "P";
    if (d_dist) {
      float f = 0.0f;
      PPK_HIP(hipMemcpy(&f, d_dist + e, 4, hipMemcpyDeviceToHost));
      if (!std::isfinite(f) || f < 0.0f) {
        v = f;
        name = "distance";
      }
    }
    if (name[0] == 'P') PPK_HIP(hipMemcpy(&v, d_P + e, 8, hipMemcpyDeviceToHost));
    what = std::string(name) + " is " + (std::isnan(v) ? "NaN" : std::isinf(v) ? "infinite" : v < 0.0 ? "negative" : "above 1");
  }
  return ppk_fail(PPK_ERR_ARG, std::string(who) + ": entry " + std::to_string(e) + " (i = " + std::to_string(i) +
                                   ", j = " + std::to_string(j) + "): " + what);
}

// the effective worker count W = min(workers, n) and the iteration count T = max(1, rint(max_iter / W)) (ppk.h)
int embed_schedule(size_t n, long long max_iter, long long workers, long long *w_eff, long long *iters) {
  if (max_iter < 1 || workers < 1 || workers > (1ll << 24))
    return ppk_fail(PPK_ERR_ARG, "ppk_embed: max_iter must be >= 1 and workers in [1, 2^24]");
  const long long w = workers < (long long)n ? workers : (long long)(n > 0 ? n : 1);
  const double t = std::nearbyint((double)max_iter / (double)w);
  if (w_eff) *w_eff = w;
  if (iters) *iters = t < 1.0 ? 1 : (long long)t;
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_embed_weights_dev(const long long *d_i, const long long *d_j, const float *d_dist, size_t n,
                                     size_t k, double perplexity, double *d_P, unsigned long long *d_c,
                                     void *stream) {
  const char *who = "ppk_embed_weights";
  int rc = check_sizes(who, n, k);
  if (rc != PPK_OK) return rc;
  if (!(perplexity > 0.0) || !std::isfinite(perplexity))
    return ppk_fail(PPK_ERR_ARG, "ppk_embed_weights: perplexity must be finite and > 0");
  if (!d_i || !d_j || !d_dist || !d_P) return ppk_fail(PPK_ERR_ARG, "ppk_embed_weights: NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n * k;
  unsigned long long *bad;
  double *part, *rms;
  if ((rc = ppk_scratch_carve(dev, SLOT_EMBED, [&](Carve &c) { c.take(bad, 1).take(part, kSumParts).take(rms, 1); })) !=
      PPK_OK)
    return rc;

  ppk_prof_stage("check", s);
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  hipLaunchKernelGGL(embed_check_kernel, dim3(grid_for(m, kThreads, 4096)), dim3(kThreads), 0, s, d_i, d_j, d_dist,
                     (const double *)nullptr, n, k, bad);
  PPK_HIP(hipGetLastError());
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 8}}, &h)) != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return bad_entry(who, d_i, d_j, d_dist, nullptr, n, k, (size_t)h[0]);
  }
  ppk_prof_stage("calibrate", s);
  hipLaunchKernelGGL(embed_sumsq_kernel, dim3(kSumParts), dim3(kThreads), 0, s, d_dist, m, part);
  hipLaunchKernelGGL(embed_rms_kernel, dim3(1), dim3(kThreads), 0, s, part, m, rms);
  hipLaunchKernelGGL(embed_calibrate_kernel, dim3(grid_for(n, kThreads, 1u << 30)), dim3(kThreads), 0, s, d_dist, n,
                     k, rms, std::log(perplexity), perplexity < (double)k ? kCalSteps : 0, d_P, d_c);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage(nullptr, s);
  return PPK_OK;
}

extern "C" int ppk_embed_dev(const long long *d_i, const long long *d_j, const double *d_P, size_t n, size_t k,
                             unsigned long long seed, long long max_iter, int n_repu, double eta0, long long workers,
                             double *d_Y, void *stream) {
  const char *who = "ppk_embed";
  int rc = check_sizes(who, n, k);
  if (rc != PPK_OK) return rc;
  if (n_repu < 0 || n_repu > 127) return ppk_fail(PPK_ERR_ARG, "ppk_embed: n_repu must be in [0, 127]");
  if (!std::isfinite(eta0) || eta0 < 0.0) return ppk_fail(PPK_ERR_ARG, "ppk_embed: eta0 must be finite and >= 0");
  long long W = 0, T = 0;
  if ((rc = embed_schedule(n, max_iter, workers, &W, &T)) != PPK_OK) return rc;
  if (!d_i || !d_j || !d_P || !d_Y) return ppk_fail(PPK_ERR_ARG, "ppk_embed: NULL array");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t m = n * k;

  // scratch: bad, high sum | q sums | Eq | c | prefix | deltas | rocprim temp
  size_t tmp_bytes = 0;
  PPK_HIP(rocprim::inclusive_scan(nullptr, tmp_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, m,
                                  rocprim::plus<unsigned long long>(), s));
  unsigned long long *bad, *c, *prefix;
  long long *qacc, *delta;
  double *Eq;
  char *tmp;
  if ((rc = ppk_scratch_carve(dev, SLOT_EMBED, [&](Carve &cv) {
         cv.take(bad, 2).take(qacc, 2).take(Eq, 1).take(c, m).take(prefix, m).take(delta, 2 * n).take(tmp, tmp_bytes);
       })) != PPK_OK)
    return rc;

  ppk_prof_stage("check", s);
  unsigned long long *high = bad + 1;
  PPK_HIP(hipMemsetAsync(bad, 0xff, 8, s));
  PPK_HIP(hipMemsetAsync(high, 0, 8, s));
  const unsigned gm = grid_for(m, kThreads, 4096);
  hipLaunchKernelGGL(embed_check_kernel, dim3(gm), dim3(kThreads), 0, s, d_i, d_j, (const float *)nullptr, d_P, n, k,
                     bad);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage("weights", s);
  hipLaunchKernelGGL(embed_quantise_kernel, dim3(gm), dim3(kThreads), 0, s, d_P, m, c, high);
  PPK_HIP(hipGetLastError());
  PPK_HIP(rocprim::inclusive_scan(tmp, tmp_bytes, c, prefix, m, rocprim::plus<unsigned long long>(), s));
  const unsigned long long *h = nullptr;
  if ((rc = ppk_read_back(dev, s, {{bad, 16}, {prefix + (m - 1), 8}}, &h)) != PPK_OK) return rc;
  if (h[0] != ~0ull) {
    ppk_prof_stage(nullptr, s);
    return bad_entry(who, d_i, d_j, nullptr, d_P, n, k, (size_t)h[0]);
  }
  if (h[1] >= kHighMax) {
    ppk_prof_stage(nullptr, s);
    return ppk_fail(PPK_ERR_ARG, "ppk_embed: the sum of the weights rint(P * 2^52) is " +
                                     std::to_string((double)h[1] * 0x1p20) + " or more (a sum of P of about " +
                                     std::to_string((double)h[1] * 0x1p-32) +
                                     "): it must stay below 2^63, a sum of P of 2048, to be summed in 64 bits");
  }
  if (h[2] == 0) {
    ppk_prof_stage(nullptr, s);
    return ppk_fail(PPK_ERR_ARG, "ppk_embed: every weight rint(P * 2^52) is 0");
  }

  ppk_prof_stage("init", s);
  const unsigned gn = grid_for(2 * n, kThreads, 4096);
  hipLaunchKernelGGL(embed_init_kernel, dim3(gn), dim3(kThreads), 0, s, n, fmix(seed ^ kInitKey), d_Y, delta, qacc,
                     Eq);
  PPK_HIP(hipGetLastError());
  const double nsq = (double)n * (double)(n - 1);
  const unsigned gw = grid_for((size_t)W, kThreads, 1u << 30);
  for (long long t = 0; t < T; ++t) {
    const double eta = T > 1 ? eta0 * std::fmax(1.0 - (double)t / (double)(T - 1), 1e-4) : eta0;
    ppk_prof_stage("step", s);
    hipLaunchKernelGGL(embed_step_kernel, dim3(gw), dim3(kThreads), 0, s, d_Y, prefix, m, d_i, d_j, n,
                       (unsigned long long)W, n_repu, iter_key(seed, t), eta, Eq, delta, qacc);
    ppk_prof_stage("apply", s);
    hipLaunchKernelGGL(embed_apply_kernel, dim3(gn), dim3(kThreads), 0, s, d_Y, delta, n, nsq, qacc, Eq);
    PPK_HIP(hipGetLastError());
    if ((t + 1) % kPoll == 0 && ppk_interrupted()) {
      ppk_prof_stage(nullptr, s);
      PPK_HIP(hipStreamSynchronize(s));
      return ppk_fail(PPK_ERR_INTERRUPTED, "ppk_embed: interrupted");
    }
  }
  ppk_prof_stage(nullptr, s);
  return PPK_OK;
}

extern "C" int ppk_embed(const long long *i, const long long *j, const float *dist, size_t n, size_t k,
                         double perplexity, unsigned long long seed, long long max_iter, int n_repu, double eta0,
                         long long workers, int device_id, double *P, double *Y) {
  int rc = check_sizes("ppk_embed", n, k);
  if (rc != PPK_OK) return rc;
  if (!i || !j || !dist || !Y) return ppk_fail(PPK_ERR_ARG, "ppk_embed: NULL array");
  if ((rc = embed_schedule(n, max_iter, workers, nullptr, nullptr)) != PPK_OK) return rc;
  const size_t m = n * k;
  long long *d_i, *d_j;
  float *d_dist;
  double *d_P, *d_Y;
  return ppk_host_frame(device_id, [&](Carve &c) {
    c.take(d_i, m).take(d_j, m).take(d_dist, m).take(d_P, m).take(d_Y, 2 * n);
  }, [&]() -> int {
    PPK_HIP(hipMemcpy(d_i, i, m * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_j, j, m * 8, hipMemcpyHostToDevice));
    PPK_HIP(hipMemcpy(d_dist, dist, m * 4, hipMemcpyHostToDevice));
    int r = ppk_embed_weights_dev(d_i, d_j, d_dist, n, k, perplexity, d_P, nullptr, nullptr);
    if (r != PPK_OK) return r;
    if ((r = ppk_embed_dev(d_i, d_j, d_P, n, k, seed, max_iter, n_repu, eta0, workers, d_Y, nullptr)) != PPK_OK)
      return r;
    if (P) PPK_HIP(hipMemcpy(P, d_P, m * 8, hipMemcpyDeviceToHost));
    PPK_HIP(hipMemcpy(Y, d_Y, 2 * n * 8, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

// Fitting the refine boundary on the device: the network counts of ONE boundary per call, which is
// what refine's local search (scipy's bounded minimiser around newNetwork, PopPUNK/refine.py:221-232,:476-548) asks for
// one evaluation after another.
//
//  - ppk_refine_score_dev : {edges, components, triangles, connected triples} of the graph of every row of a resident
//    condensed float32 [n(n-1)/2][2] matrix with line_dist <= 0 (edgeThreshold's rows, inclusive).  No edge list is
//    formed: the graph lives as a symmetric n x n BIT MATRIX in scratch (1/32 of the distance matrix), which a
//    condensed matrix addresses directly -- row k is the pair (i, j), bit j of bit-row i.
//    Stages (ppk_prof_stage names):
//      refine_classify   one pass over the matrix: the un-fused ppk_line_dist of every row; a passing row sets its two
//                        bits and links its two roots in a lock-free union-find (the rule of the network sweep's
//                        components stage: a root links under the smaller root by CAS, each success removes a component)
//      refine_degrees    one wave per vertex: degree = popcount of its bit-row; edges = sum d / 2, triples = sum C(d, 2)
//      refine_triangles  one workgroup per vertex u, one wave per neighbour v > u: popcount(row u & row v) over the
//                        bits above v -- every triangle u < v < w once
//    All sums are integers added with integer atomics: the result does not depend on arrival order.  The call's one
//    synchronisation reads the four counts back.
//  - ppk_refine_local_* : the same counts for every line BETWEEN two nested lines (a bracket), from a handle that has
//    done the common work once.  Create sorts the rows into base (inside the lower line by more than the 2^-20 relative
//    margin of ppk_iterate.hip's window argument: an edge of every line of the bracket), never (outside the upper line
//    by more than the margin) and candidates (the rest, compacted in row order with their coordinates and (i, j)), and
//    keeps the base graph resident: its bit matrix, union-find parents, degrees, edge and triangle counts.  An
//    evaluation tests only the candidates (exact ppk_line_dist <= 0; the passing set P), gives P a bit matrix of its
//    own in scratch, links P into a COPY of the base parents, and counts
//      triples    sum over vertices of C(deg_B + deg_P, 2)
//      triangles  T_B + the triangles with at least one P edge.  With G = B u P, one wave per P edge (u, v) forms
//                 S1 = |N_G(u) & N_G(v)|, S2 = |N_P(u) & N_G(v)| + |N_G(u) & N_P(v)|, S3 = |N_P(u) & N_P(v)|; summed
//                 over P a triangle with 1, 2, 3 P edges contributes (1, 0, 0), (2, 2, 0), (3, 6, 3), so
//                 S1 - S2 / 2 + S3 / 3 counts each exactly once (both divisions are exact).
//    An evaluation writes nothing into the handle.
#include <cmath>
#include <rocprim/device/device_scan.hpp>

#include "ppk_internal.h"

struct ppk_refine_local {
  int device, slope;
  size_t n, n_rows, words;       // vertices, matrix rows, 64-bit words per bit-row
  float lo[2], hi[2];
  unsigned long long n_base, n_cand, n_never;
  char *d_block;                 // one allocation: the base graph
  unsigned long long *d_bits;    // [n][words]
  int *d_parent;                 // [n]
  unsigned *d_deg;               // [n]
  unsigned long long *d_cnt;     // counters of the base graph (C_*)
  char *d_cand;                  // one allocation: the candidates
  float2 *d_xy;                  // [n_cand]
  int *d_ci, *d_cj;              // [n_cand]
};

namespace {

constexpr int kThreads = 256;
constexpr int kChunkSteps = 16;                      // a compaction chunk: kChunkSteps * kThreads rows
constexpr size_t kChunk = (size_t)kChunkSteps * kThreads;
enum { C_LINKS = 0, C_DEG2, C_TRIPLES, C_TRI, C_P, C_S1, C_S2, C_S3, C_BASE, C_CAND, C_NEVER, C_LEN = 16 };
enum { CLASS_BASE = 0, CLASS_CAND = 1, CLASS_NEVER = 2 };

__device__ __forceinline__ void set_edge(unsigned long long *bits, size_t words, int i, int j) {
  atomicOr(bits + (size_t)i * words + ((unsigned)j >> 6), 1ull << (j & 63));
  atomicOr(bits + (size_t)j * words + ((unsigned)i >> 6), 1ull << (i & 63));
}

__global__ void __launch_bounds__(kThreads) rf_parent_init_kernel(int *parent, size_t n) {
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x)
    parent[v] = (int)v;
}

// ---- refine_classify ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) rf_classify_kernel(const float2 *__restrict__ dist, size_t n_rows, size_t n,
                                                               size_t words, int slope, float x_max, float y_max,
                                                               unsigned long long *bits, int *parent,
                                                               unsigned long long *cnt) {
  unsigned long long links = 0;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += (size_t)gridDim.x * blockDim.x) {
    const float2 d = dist[k];
    if (ppk_line_dist(d.x, d.y, x_max, y_max, slope) <= 0.0f) {
      int i, j;
      cond_pair(k, n, i, j);
      set_edge(bits, words, i, j);
      links += uf_union(parent, i, j);
    }
  }
  wave_add(cnt + C_LINKS, links);
}

// ---- refine_degrees: one wave per vertex -------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) rf_degree_kernel(const unsigned long long *__restrict__ bits, size_t n,
                                                             size_t words, unsigned *deg, unsigned long long *cnt) {
  const unsigned lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long deg2 = 0, triples = 0;      // (lane 0 holds the wave's sums)
  for (size_t v = wave; v < n; v += n_waves) {
    unsigned long long c = 0;
    for (size_t w = lane; w < words; w += 64) c += (unsigned)__popcll(bits[v * words + w]);
    c = wave_sum(c);
    if (lane == 0) {
      if (deg) deg[v] = (unsigned)c;
      deg2 += c;
      triples += c * (c - 1) / 2;
    }
  }
  if (lane == 0) {
    if (deg2) atomicAdd(cnt + C_DEG2, deg2);
    if (triples) atomicAdd(cnt + C_TRIPLES, triples);
  }
}

// ---- refine_triangles: one workgroup per u, its waves take the neighbours v > u in turn ---------------------------
__global__ void __launch_bounds__(kThreads) rf_triangles_kernel(const unsigned long long *__restrict__ bits, size_t n,
                                                                size_t words, unsigned long long *cnt) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  unsigned long long tri = 0;
  for (size_t u = blockIdx.x; u + 2 < n; u += gridDim.x) {
    const unsigned long long *ru = bits + u * words;
    unsigned turn = 0;
    for (size_t q = u >> 6; q < words; ++q) {
      unsigned long long b = ru[q];                              // (wave-uniform)
      if (q == (u >> 6)) b &= ~((2ull << (u & 63)) - 1ull);      // bits above u; u = 63 mod 64: none of this word
      while (b) {
        const unsigned t = (unsigned)__builtin_ctzll(b);
        b &= b - 1;
        if (turn++ % n_waves != wave) continue;
        const size_t v = q * 64 + t;
        const unsigned long long *rv = bits + v * words;
        for (size_t x = (v >> 6) + lane; x < words; x += 64) {
          unsigned long long c = ru[x] & rv[x];
          if (x == (v >> 6)) c &= ~((2ull << (v & 63)) - 1ull);
          tri += (unsigned)__popcll(c);
        }
      }
    }
  }
  wave_add(cnt + C_TRI, tri);
}

__global__ void rf_stats_kernel(const unsigned long long *cnt, long long n, long long *stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  stats[0] = (long long)(cnt[C_DEG2] / 2);
  stats[1] = n - (long long)cnt[C_LINKS];
  stats[2] = (long long)cnt[C_TRI];
  stats[3] = (long long)cnt[C_TRIPLES];
}

// ---- the bracket: create -----------------------------------------------------------------------------------------
struct Bracket {
  int slope;
  float xl, yl, xh, yh;
  float cl_in, ch_out;      // slope 2: fl(c_lo (1 - 2^-20)), fl(c_hi (1 + 2^-20))
};

// Base: within the lower line and every line around it.  Never: outside the upper line and every line inside it.
// Slope 2 (both lines with intercepts >= 2^-40, finite, nested): the window argument of ppk_iterate.hip, which needs
// x, y >= 0 and only that the intercepts of the later line are no smaller (base) / no larger (never).  Slopes 0 and 1:
// side = fl(x - x_max) has the sign of the exact difference, so x <= x_lo is within every x_max >= x_lo and x > x_hi
// outside every x_max <= x_hi.  A NaN coordinate (any slope) and a negative one (slope 2) are candidates.
__device__ __forceinline__ int classify_row(float x, float y, const Bracket &b) {
  if (b.slope == 0) return x <= b.xl ? CLASS_BASE : (x > b.xh ? CLASS_NEVER : CLASS_CAND);
  if (b.slope == 1) return y <= b.yl ? CLASS_BASE : (y > b.yh ? CLASS_NEVER : CLASS_CAND);
  if (!(x >= 0.0f && y >= 0.0f)) return CLASS_CAND;
  const float al = __fadd_rn(__fmul_rn(y, b.xl), __fmul_rn(x, b.yl));
  if (al < b.cl_in) return CLASS_BASE;
  const float ah = __fadd_rn(__fmul_rn(y, b.xh), __fmul_rn(x, b.yh));
  if (ah > b.ch_out) return CLASS_NEVER;
  return CLASS_CAND;
}

// pass 1: the base graph, and the candidates of every chunk counted
__global__ void __launch_bounds__(kThreads) rl_split_kernel(const float2 *__restrict__ dist, size_t n_rows, size_t n,
                                                            size_t words, Bracket br, unsigned long long *bits,
                                                            int *parent, unsigned long long *chunk_cnt, size_t n_chunks,
                                                            unsigned long long *cnt) {
  __shared__ unsigned s_cand;
  unsigned long long links = 0, base = 0, never = 0;
  for (size_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    if (threadIdx.x == 0) s_cand = 0;
    __syncthreads();
    unsigned cand = 0;
    for (int st = 0; st < kChunkSteps; ++st) {
      const size_t k = c * kChunk + (size_t)st * kThreads + threadIdx.x;
      if (k >= n_rows) break;
      const float2 d = dist[k];
      const int cls = classify_row(d.x, d.y, br);
      if (cls == CLASS_BASE) {
        int i, j;
        cond_pair(k, n, i, j);
        set_edge(bits, words, i, j);
        links += uf_union(parent, i, j);
        ++base;
      } else if (cls == CLASS_CAND) {
        ++cand;
      } else {
        ++never;
      }
    }
    if (cand) atomicAdd(&s_cand, cand);
    __syncthreads();
    if (threadIdx.x == 0) chunk_cnt[c] = s_cand;
    __syncthreads();
  }
  wave_add(cnt + C_LINKS, links);
  wave_add(cnt + C_BASE, base);
  wave_add(cnt + C_NEVER, never);
}

// pass 2: the candidates in row order (chunk_off = the exclusive scan of chunk_cnt)
__global__ void __launch_bounds__(kThreads) rl_gather_kernel(const float2 *__restrict__ dist, size_t n_rows, size_t n,
                                                             Bracket br, const unsigned long long *chunk_off,
                                                             size_t n_chunks, size_t cap, float2 *xy, int *ci, int *cj) {
  __shared__ unsigned s_wave[kThreads / 64];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (size_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    size_t pos = (size_t)chunk_off[c];
    for (int st = 0; st < kChunkSteps; ++st) {
      const size_t k0 = c * kChunk + (size_t)st * kThreads;
      if (k0 >= n_rows) break;                 // (workgroup-uniform)
      const size_t k = k0 + threadIdx.x;
      float2 d = make_float2(0.0f, 0.0f);
      bool is = false;
      if (k < n_rows) {
        d = dist[k];
        is = classify_row(d.x, d.y, br) == CLASS_CAND;
      }
      const unsigned long long m = __ballot(is);
      if (lane == 0) s_wave[wave] = (unsigned)__popcll(m);
      __syncthreads();
      size_t at = pos;
      unsigned total = 0;
      for (unsigned w = 0; w < kThreads / 64; ++w) {
        if (w < wave) at += s_wave[w];
        total += s_wave[w];
      }
      if (is) {
        at += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (at < cap) {
          int i, j;
          cond_pair(k, n, i, j);
          xy[at] = d;
          ci[at] = i;
          cj[at] = j;
        }
      }
      pos += total;
      __syncthreads();
    }
  }
}

// ---- the bracket: evaluate ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) rl_test_kernel(const float2 *__restrict__ xy, const int *__restrict__ ci,
                                                           const int *__restrict__ cj, size_t m, int slope, float x_max,
                                                           float y_max, size_t words, unsigned long long *bits_p,
                                                           int *parent, unsigned *deg_p, unsigned char *pass,
                                                           unsigned long long *cnt) {
  unsigned long long links = 0, np = 0;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (size_t)gridDim.x * blockDim.x) {
    const float2 d = xy[k];
    const bool in = ppk_line_dist(d.x, d.y, x_max, y_max, slope) <= 0.0f;
    pass[k] = in ? 1 : 0;
    if (in) {
      const int i = ci[k], j = cj[k];
      set_edge(bits_p, words, i, j);
      atomicAdd(deg_p + i, 1u);
      atomicAdd(deg_p + j, 1u);
      links += uf_union(parent, i, j);
      ++np;
    }
  }
  wave_add(cnt + C_LINKS, links);
  wave_add(cnt + C_P, np);
}

__global__ void __launch_bounds__(kThreads) rl_triples_kernel(const unsigned *__restrict__ deg_b,
                                                              const unsigned *__restrict__ deg_p, size_t n,
                                                              unsigned long long *cnt) {
  unsigned long long t = 0;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long d = (unsigned long long)deg_b[v] + deg_p[v];
    t += d * (d - 1) / 2;
  }
  wave_add(cnt + C_TRIPLES, t);
}

// one wave per candidate (grid-stride), the passing ones only
__global__ void __launch_bounds__(kThreads) rl_triangles_kernel(const unsigned long long *__restrict__ bits_b,
                                                                const unsigned long long *__restrict__ bits_p,
                                                                size_t words, const int *__restrict__ ci,
                                                                const int *__restrict__ cj,
                                                                const unsigned char *__restrict__ pass, size_t m,
                                                                unsigned long long *cnt) {
  const unsigned lane = threadIdx.x & 63;
  const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long s1 = 0, s2 = 0, s3 = 0;
  for (size_t k = wave; k < m; k += n_waves) {
    if (!pass[k]) continue;                    // (wave-uniform)
    const size_t u = (size_t)ci[k] * words, v = (size_t)cj[k] * words;
    for (size_t x = lane; x < words; x += 64) {
      const unsigned long long pu = bits_p[u + x], pv = bits_p[v + x];
      const unsigned long long gu = bits_b[u + x] | pu, gv = bits_b[v + x] | pv;
      s1 += (unsigned)__popcll(gu & gv);
      s2 += (unsigned)__popcll(pu & gv) + (unsigned)__popcll(gu & pv);
      s3 += (unsigned)__popcll(pu & pv);
    }
  }
  wave_add(cnt + C_S1, s1);
  wave_add(cnt + C_S2, s2);
  wave_add(cnt + C_S3, s3);
}

// base: the handle's counters (links, 2 E_B, T_B); ev: this evaluation's
__global__ void rl_stats_kernel(const unsigned long long *base, const unsigned long long *ev, long long n,
                                long long *stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  stats[0] = (long long)(base[C_DEG2] / 2 + ev[C_P]);
  stats[1] = n - (long long)(base[C_LINKS] + ev[C_LINKS]);
  stats[2] = (long long)(base[C_TRI] + ev[C_S1] - ev[C_S2] / 2 + ev[C_S3] / 3);
  stats[3] = (long long)ev[C_TRIPLES];
}

// ---- host side ---------------------------------------------------------------------------------------------------
// the matrix of a refine call, checked: *n = its sample count
int check_matrix(const std::string &who, const float *d_dist, size_t n_rows, int slope, size_t *n) {
  if (!d_dist) return ppk_fail(PPK_ERR_ARG, who + ": NULL distance matrix");
  if (reinterpret_cast<uintptr_t>(d_dist) & 7) return ppk_fail(PPK_ERR_ARG, who + ": the matrix must be 8-byte aligned");
  if (slope < 0 || slope > 2) return ppk_fail(PPK_ERR_ARG, who + ": slope must be 0, 1 or 2");
  if (n_rows == 0) return ppk_fail(PPK_ERR_ARG, who + ": no rows");
  if (int rc = ppk_condensed_samples(n_rows, n, who + ": ")) return rc;
  if (*n >= ((size_t)1 << 31)) return ppk_fail(PPK_ERR_ARG, who + ": n_vertices must be < 2^31");
  return PPK_OK;
}

// degrees (deg nullable), then triangles, of a finished bit matrix, into cnt
int launch_graph_counts(const unsigned long long *bits, size_t n, size_t words, unsigned *deg, unsigned long long *cnt,
                        hipStream_t s) {
  ppk_prof_stage("refine_degrees", s);
  hipLaunchKernelGGL(rf_degree_kernel, dim3(grid_for(n, kThreads / 64, 8192)), dim3(kThreads), 0, s, bits, n, words, deg,
                     cnt);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage("refine_triangles", s);
  hipLaunchKernelGGL(rf_triangles_kernel, dim3(grid_for(n, 1, 1u << 20)), dim3(kThreads), 0, s, bits, n, words, cnt);
  PPK_HIP(hipGetLastError());
  return PPK_OK;
}

int check_handle(const ppk_refine_local *h, const char *who) {
  if (!h || !h->d_block) return ppk_fail(PPK_ERR_ARG, std::string(who) + ": NULL handle");
  return PPK_OK;
}

}  // namespace

extern "C" int ppk_refine_score_dev(const float *d_dist, size_t n_rows, int slope, float x_max, float y_max,
                                    long long *d_stats, void *stream) {
  const std::string who = "ppk_refine_score";
  size_t n = 0;
  if (int rc = check_matrix(who, d_dist, n_rows, slope, &n)) return rc;
  if (!d_stats) return ppk_fail(PPK_ERR_ARG, who + ": NULL stats");
  if (x_max != x_max || y_max != y_max) return ppk_fail(PPK_ERR_ARG, who + ": the line is NaN");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  const size_t words = (n + 63) / 64;
  unsigned long long *bits, *cnt;
  int *parent;
  int rc = ppk_scratch_carve(dev, SLOT_REFINE, [&](Carve &c) { c.take(cnt, C_LEN).take(parent, n).take(bits, n * words); });
  if (rc != PPK_OK) return rc;
  ppk_prof_stage("refine_classify", s);
  PPK_HIP(hipMemsetAsync(cnt, 0, C_LEN * 8, s));
  PPK_HIP(hipMemsetAsync(bits, 0, n * words * 8, s));
  hipLaunchKernelGGL(rf_parent_init_kernel, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, s, parent, n);
  hipLaunchKernelGGL(rf_classify_kernel, dim3(grid_for(n_rows, kThreads * 8, 2048)), dim3(kThreads), 0, s,
                     reinterpret_cast<const float2 *>(d_dist), n_rows, n, words, slope, x_max, y_max, bits, parent, cnt);
  PPK_HIP(hipGetLastError());
  if ((rc = launch_graph_counts(bits, n, words, nullptr, cnt, s)) != PPK_OK) {
    ppk_prof_stage(nullptr, s);
    return rc;
  }
  hipLaunchKernelGGL(rf_stats_kernel, dim3(1), dim3(64), 0, s, cnt, (long long)n, d_stats);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage(nullptr, s);
  const unsigned long long *h = nullptr;
  return ppk_read_back(dev, s, {{d_stats, 32}}, &h);      // the one synchronisation: the counts are there on return
}

extern "C" int ppk_refine_score(const float *dist, size_t n_rows, int slope, float x_max, float y_max, int device_id,
                                long long *stats) {
  if (!dist || !stats) return ppk_fail(PPK_ERR_ARG, "ppk_refine_score: NULL array");
  float *d_dist;
  long long *d_stats;
  return ppk_host_frame(device_id, [&](Carve &c) { c.take(d_dist, 2 * n_rows).take(d_stats, 4); }, [&]() -> int {
    if (n_rows) PPK_HIP(hipMemcpy(d_dist, dist, n_rows * 8, hipMemcpyHostToDevice));
    const int rc = ppk_refine_score_dev(d_dist, n_rows, slope, x_max, y_max, d_stats, nullptr);
    if (rc != PPK_OK) return rc;
    PPK_HIP(hipMemcpy(stats, d_stats, 32, hipMemcpyDeviceToHost));
    return PPK_OK;
  });
}

extern "C" void ppk_refine_local_destroy(ppk_refine_local *h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  if (h->d_block) (void)hipFree(h->d_block);
  if (h->d_cand) (void)hipFree(h->d_cand);
  delete h;
}

extern "C" int ppk_refine_local_create_dev(const float *d_dist, size_t n_rows, int slope, float x_lo, float y_lo,
                                           float x_hi, float y_hi, void *stream, ppk_refine_local **out) {
  const std::string who = "ppk_refine_local_create";
  size_t n = 0;
  if (!out) return ppk_fail(PPK_ERR_ARG, who + ": NULL handle pointer");
  *out = nullptr;
  if (int rc = check_matrix(who, d_dist, n_rows, slope, &n)) return rc;
  // nested: for slope 0 only the x pair matters, for slope 1 only the y pair; slope 2 also needs what the margin
  // argument needs, finite intercepts of at least 2^-40 (which keeps every line of the bracket off the sqrt branch)
  const float tiny = 0x1p-40f;
  bool nested;
  if (slope == 0) nested = x_lo <= x_hi;
  else if (slope == 1) nested = y_lo <= y_hi;
  else nested = x_lo <= x_hi && y_lo <= y_hi && x_lo >= tiny && y_lo >= tiny && std::isfinite(x_hi) && std::isfinite(y_hi);
  if (!nested) {
    ppk_set_error(who + ": the two lines are not nested");
    return PPK_REFINE_NOT_NESTED;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int dev = 0;
  PPK_HIP(hipGetDevice(&dev));
  PpkCall call(dev, s);
  Bracket br{slope, x_lo, y_lo, x_hi, y_hi, 0.0f, 0.0f};
  br.cl_in = (x_lo * y_lo) * (1.0f - 0x1p-20f);
  br.ch_out = (x_hi * y_hi) * (1.0f + 0x1p-20f);

  std::unique_ptr<ppk_refine_local, void (*)(ppk_refine_local *)> h(new ppk_refine_local(), ppk_refine_local_destroy);
  h->device = dev;
  h->slope = slope;
  h->n = n;
  h->n_rows = n_rows;
  h->words = (n + 63) / 64;
  h->lo[0] = x_lo, h->lo[1] = y_lo, h->hi[0] = x_hi, h->hi[1] = y_hi;
  h->d_block = h->d_cand = nullptr;
  const size_t words = h->words;
  Carve hc;
  auto handle_layout = [&](Carve &c) { c.take(h->d_cnt, C_LEN).take(h->d_parent, n).take(h->d_deg, n).take(h->d_bits, n * words); };
  handle_layout(hc);
  PPK_HIP(hipMalloc(reinterpret_cast<void **>(&h->d_block), hc.at));
  hc = Carve{h->d_block};
  handle_layout(hc);

  const size_t n_chunks = (n_rows + kChunk - 1) / kChunk;
  size_t scan_tmp = 0;
  PPK_HIP(rocprim::exclusive_scan(nullptr, scan_tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr, 0ull,
                                  n_chunks + 1, rocprim::plus<unsigned long long>(), s));
  unsigned long long *chunk_cnt, *chunk_off;
  char *d_tmp;
  int rc = ppk_scratch_carve(dev, SLOT_REFINE, [&](Carve &c) {
    c.take(chunk_cnt, n_chunks + 1).take(chunk_off, n_chunks + 1).take(d_tmp, scan_tmp + 16);
  });
  if (rc != PPK_OK) return rc;

  ppk_prof_stage("refine_split", s);
  PPK_HIP(hipMemsetAsync(h->d_cnt, 0, C_LEN * 8, s));
  PPK_HIP(hipMemsetAsync(h->d_bits, 0, n * words * 8, s));
  PPK_HIP(hipMemsetAsync(chunk_cnt + n_chunks, 0, 8, s));
  hipLaunchKernelGGL(rf_parent_init_kernel, dim3(grid_for(n, kThreads, 4096)), dim3(kThreads), 0, s, h->d_parent, n);
  const unsigned g_chunks = grid_for(n_chunks, 1, 4096);
  const float2 *dist2 = reinterpret_cast<const float2 *>(d_dist);
  hipLaunchKernelGGL(rl_split_kernel, dim3(g_chunks), dim3(kThreads), 0, s, dist2, n_rows, n, words, br, h->d_bits,
                     h->d_parent, chunk_cnt, n_chunks, h->d_cnt);
  PPK_HIP(hipGetLastError());
  size_t tb = scan_tmp;
  PPK_HIP(rocprim::exclusive_scan(d_tmp, tb, chunk_cnt, chunk_off, 0ull, n_chunks + 1, rocprim::plus<unsigned long long>(), s));
  const unsigned long long *w = nullptr;
  if ((rc = ppk_read_back(dev, s, {{chunk_off + n_chunks, 8}, {h->d_cnt + C_BASE, 8}, {h->d_cnt + C_NEVER, 8}}, &w)) != PPK_OK) {
    ppk_prof_stage(nullptr, s);
    return rc;
  }
  h->n_cand = w[0];
  h->n_base = w[1];
  h->n_never = w[2];
  const size_t m = (size_t)h->n_cand;
  Carve cc;
  auto cand_layout = [&](Carve &c) { c.take(h->d_xy, m + 1).take(h->d_ci, m + 1).take(h->d_cj, m + 1); };
  cand_layout(cc);
  PPK_HIP(hipMalloc(reinterpret_cast<void **>(&h->d_cand), cc.at));
  cc = Carve{h->d_cand};
  cand_layout(cc);
  if (m) {
    hipLaunchKernelGGL(rl_gather_kernel, dim3(g_chunks), dim3(kThreads), 0, s, dist2, n_rows, n, br, chunk_off, n_chunks,
                       m, h->d_xy, h->d_ci, h->d_cj);
    PPK_HIP(hipGetLastError());
  }
  rc = launch_graph_counts(h->d_bits, n, words, h->d_deg, h->d_cnt, s);
  ppk_prof_stage(nullptr, s);
  if (rc != PPK_OK) return rc;
  PPK_HIP(hipStreamSynchronize(s));      // the handle is complete on return, whatever stream evaluates it
  *out = h.release();
  return PPK_OK;
}

extern "C" int ppk_refine_local_stats(const ppk_refine_local *h, unsigned long long *split) {
  if (int rc = check_handle(h, "ppk_refine_local_stats")) return rc;
  if (!split) return ppk_fail(PPK_ERR_ARG, "ppk_refine_local_stats: NULL argument");
  split[0] = h->n_base;
  split[1] = h->n_cand;
  split[2] = h->n_never;
  return PPK_OK;
}

extern "C" int ppk_refine_local_eval_dev(const ppk_refine_local *h, float x_max, float y_max, long long *d_stats,
                                         void *stream) {
  const std::string who = "ppk_refine_local_eval";
  if (int rc = check_handle(h, who.c_str())) return rc;
  if (!d_stats) return ppk_fail(PPK_ERR_ARG, who + ": NULL stats");
  const bool x_in = x_max >= h->lo[0] && x_max <= h->hi[0], y_in = y_max >= h->lo[1] && y_max <= h->hi[1];
  if ((h->slope != 1 && !x_in) || (h->slope != 0 && !y_in)) return ppk_fail(PPK_ERR_ARG, who + ": the line is outside the bracket");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PPK_ENTER_DEVICE(guard, h->device);
  const int dev = h->device;
  PpkCall call(dev, s);
  const size_t n = h->n, words = h->words, m = (size_t)h->n_cand;
  unsigned long long *bits_p, *cnt;
  int *parent;
  unsigned *deg_p;
  unsigned char *pass;
  int rc = ppk_scratch_carve(dev, SLOT_REFINE, [&](Carve &c) {
    c.take(cnt, C_LEN).take(parent, n).take(deg_p, n).take(pass, m + 1).take(bits_p, n * words);
  });
  if (rc != PPK_OK) return rc;
  ppk_prof_stage("refine_local_test", s);
  PPK_HIP(hipMemsetAsync(cnt, 0, C_LEN * 8, s));
  PPK_HIP(hipMemsetAsync(deg_p, 0, n * 4, s));
  PPK_HIP(hipMemcpyAsync(parent, h->d_parent, n * 4, hipMemcpyDeviceToDevice, s));
  if (m) {
    PPK_HIP(hipMemsetAsync(bits_p, 0, n * words * 8, s));
    hipLaunchKernelGGL(rl_test_kernel, dim3(grid_for(m, kThreads * 2, 2048)), dim3(kThreads), 0, s, h->d_xy, h->d_ci,
                       h->d_cj, m, h->slope, x_max, y_max, words, bits_p, parent, deg_p, pass, cnt);
    PPK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rl_triples_kernel, dim3(grid_for(n, kThreads, 2048)), dim3(kThreads), 0, s, h->d_deg, deg_p, n, cnt);
  PPK_HIP(hipGetLastError());
  if (m) {
    ppk_prof_stage("refine_local_triangles", s);
    hipLaunchKernelGGL(rl_triangles_kernel, dim3(grid_for(m, kThreads / 64, 8192)), dim3(kThreads), 0, s, h->d_bits,
                       bits_p, words, h->d_ci, h->d_cj, pass, m, cnt);
    PPK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rl_stats_kernel, dim3(1), dim3(64), 0, s, h->d_cnt, cnt, (long long)n, d_stats);
  PPK_HIP(hipGetLastError());
  ppk_prof_stage(nullptr, s);
  const unsigned long long *w = nullptr;
  return ppk_read_back(dev, s, {{d_stats, 32}}, &w);      // the evaluation's one synchronisation
}

// Host-side check of the arithmetic in poppunk_amd/csrc/ppk_device.h that the host can run: built and run by
// test_device_helpers_host.py (host only, under the undefined-behaviour and address sanitizers).  Exit status 0 and
// the count of checks on stdout, or the first failures on stderr and exit status 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../poppunk_amd/csrc/ppk_device.h"

static std::string g_msg;
int ppk_fail(int code, const std::string &msg) {      // the library's is in ppk_api.hip
  g_msg = msg;
  return code;
}

static unsigned long long g_checks = 0;
static int g_bad = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond) && ++g_bad <= 20) {                       \
      std::fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
    }                                                     \
  } while (0)

static const size_t kLarge[] = {46341, 65536, 100000, 1000003, 16777217, 33554432};

static void condensed() {
  for (size_t n = 2; n <= 300; ++n) {
    const size_t rows = n * (n - 1) / 2;
    CHECK(ppk_samples_of_rows(rows) == n, "samples_of_rows(%zu) != %zu", rows, n);
    for (size_t k = 0; k < rows; ++k) {
      int i = -1, j = -1;
      cond_pair(k, n, i, j);
      CHECK(0 <= i && i < j && (size_t)j < n && cond_index((size_t)i, (size_t)j, n) == k, "n %zu row %zu -> (%d, %d)", n, k,
            i, j);
    }
  }
  for (size_t n : kLarge) {
    CHECK(ppk_samples_of_rows(n * (n - 1) / 2) == n, "samples_of_rows at n = %zu", n);
    for (size_t i : {(size_t)0, (size_t)1, n / 3, n / 2, n - 3, n - 2}) {
      const size_t first = cond_row_start(i, n), last = cond_row_start(i + 1, n) - 1;
      CHECK(cond_row_i(first, n) == i, "n %zu: first row of i = %zu", n, i);
      CHECK(cond_row_i(last, n) == i, "n %zu: last row of i = %zu", n, i);
      CHECK(cond_index(i, i + 1, n) == first && cond_index(i, n - 1, n) == last, "n %zu: cond_index of i = %zu", n, i);
    }
  }
  // the check's three message texts
  size_t n = 0;
  CHECK(ppk_condensed_samples(10, &n) == PPK_OK && n == 5, "10 rows are 5 samples");
  CHECK(ppk_condensed_samples(11, &n) == PPK_ERR_ARG &&
            g_msg == "row count is not n(n-1)/2 for any n (self/condensed matrix expected)",
        "message: %s", g_msg.c_str());
  CHECK(ppk_condensed_samples(11, &n, "ppk_refine_score: ") == PPK_ERR_ARG &&
            g_msg == "ppk_refine_score: row count is not n(n-1)/2 for any n (self/condensed matrix expected)",
        "message: %s", g_msg.c_str());
  CHECK(ppk_condensed_samples(11, &n, "ppk_edge_weights: ", "self matrix") == PPK_ERR_ARG &&
            g_msg == "ppk_edge_weights: row count is not n(n-1)/2 for any n (self matrix expected)",
        "message: %s", g_msg.c_str());
}

static void lower_triangle() {
  for (size_t e = 0; e < tri(300); ++e) {
    const size_t a = row_of(e), b = e - tri(a);
    CHECK(a >= 1 && b < a && tidx(a, b) == e && tidx(b, a) == e, "entry %zu -> (%zu, %zu)", e, a, b);
  }
  for (size_t n : kLarge)
    for (size_t a : {(size_t)1, (size_t)2, n / 3, n / 2, n - 2, n - 1}) {
      CHECK(row_of(tri(a)) == a, "n %zu: first entry of row %zu", n, a);
      CHECK(row_of(tri(a + 1) - 1) == a, "n %zu: last entry of row %zu", n, a);
    }
}

static unsigned bits_of(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

static void order_keys() {
  const float inf = std::numeric_limits<float>::infinity(), tiny = std::numeric_limits<float>::denorm_min();
  const float v[] = {-inf, -1.0f, -tiny, -0.0f, 0.0f, tiny, 1.0f, inf};
  for (int i = 0; i + 1 < 8; ++i) {
    const bool zeros = v[i] == 0.0f && v[i + 1] == 0.0f;
    if (zeros) CHECK(ord_of(v[i]) == ord_of(v[i + 1]), "the two zeros share a folded key");
    else CHECK(ord_of(v[i]) < ord_of(v[i + 1]), "folded keys of %g and %g", v[i], v[i + 1]);
    CHECK(ord_raw(v[i]) < ord_raw(v[i + 1]), "raw keys of %g and %g", v[i], v[i + 1]);
  }
  for (float f : v) {
    const unsigned want = bits_of(f) == 0x80000000u ? 0u : bits_of(f);      // -0.0 comes back as +0.0
    CHECK(bits_of(ord_inv(ord_of(f))) == want, "ord_inv(ord_of(%g))", f);
  }
  CHECK(ord_raw(-0.0f) < ord_raw(0.0f), "the raw key puts -0.0 below +0.0");
}

static void host_only() {
  const size_t at[] = {0, 1, 2, 3, 4, 5, ((size_t)1 << 31) - 1, (size_t)1 << 31};
  const int want[] = {0, 0, 1, 2, 2, 3, 31, 31};
  for (int i = 0; i < 8; ++i) CHECK(ceil_log2(at[i]) == want[i], "ceil_log2(%zu) = %d", at[i], ceil_log2(at[i]));
  double L[3] = {0, 0, 0};
  CHECK(chol2(4.0, 2.0, 5.0, L) && L[0] == 2.0 && L[1] == 1.0 && L[2] == 2.0, "chol2 of [[4, 2], [2, 5]]");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(!chol2(0.0, 0.0, 1.0, L) && !chol2(-1.0, 0.0, 1.0, L), "chol2: non-positive first pivot");
  CHECK(!chol2(1.0, 2.0, 4.0, L) && !chol2(1.0, 3.0, 4.0, L), "chol2: non-positive second pivot");
  CHECK(!chol2(nan, 0.0, 1.0, L) && !chol2(1.0, nan, 1.0, L) && !chol2(1.0, 0.0, nan, L), "chol2: NaN");
  const double mean[2] = {3.0, 5.0}, F[3] = {2.0, 1.0, 4.0};
  double lin[5];
  ppk_lin_of(mean, F, 0.5, 0.25, lin);
  CHECK(lin[0] == 0.5 && lin[1] == -1.5 && lin[2] == 0.25 && lin[3] == -0.25 && lin[4] == -1.25, "ppk_lin_of");
}

int main() {
  condensed();
  lower_triangle();
  order_keys();
  host_only();
  std::printf("%llu checks, %d wrong\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}

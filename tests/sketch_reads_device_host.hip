// Host-side check of the read-sample functions of poppunk_amd/csrc/ppk_device.h (the count table's row index and
// default bits, the length estimate) against values written by tests/sketch_reads_model.py: built and run by
// test_sketch_reads_host.py (host only, under the undefined-behaviour and address sanitizers).  argv[1]: a text file of
//   I <hash, hex> <row> <bits> <index>         one row index
//   D <codes> <bits>                           the default bits of a sample of that many codes
//   L <adm_occ> <filled> <win_occ> <length>    the length estimate
//   T <bits> <min_count> <n> <hashes, hex ...> a table of 2 rows of 2^bits counters filled from the n hashes; then
//   A <0 / 1 per hash>                         which of them the table admits
// Exit status 0 and the count of checks on stdout, or the first failures on stderr and exit status 1.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

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

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <records>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::string line;
  std::vector<uint64_t> hashes;
  int t_bits = 0;
  uint32_t t_min = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    char kind = 0;
    ls >> kind;
    if (kind == 'I') {
      uint64_t h = 0;
      int row = 0, bits = 0;
      uint32_t index = 0;
      ls >> std::hex >> h >> std::dec >> row >> bits >> index;
      const uint32_t mine = ppk_sketch_count_index(h, row, bits);
      CHECK(mine == index && mine < ((uint32_t)1 << bits), "index of %016" PRIx64 " row %d bits %d: %u, model %u", h, row,
            bits, mine, index);
    } else if (kind == 'D') {
      long long codes = 0;
      int bits = 0;
      ls >> codes >> bits;
      CHECK(ppk_sketch_count_bits(codes) == bits, "default bits of %lld codes: %d, model %d", codes,
            ppk_sketch_count_bits(codes), bits);
    } else if (kind == 'L') {
      unsigned long long adm = 0, filled = 0, win = 0;
      long long length = 0;
      ls >> adm >> filled >> win >> length;
      CHECK(ppk_sketch_reads_length(adm, filled, win) == length, "length of %llu %llu %llu: %lld, model %lld", adm, filled,
            win, ppk_sketch_reads_length(adm, filled, win), length);
    } else if (kind == 'T') {
      size_t n = 0;
      ls >> t_bits >> t_min >> n;
      hashes.assign(n, 0);
      for (size_t i = 0; i < n; ++i) ls >> std::hex >> hashes[i];
    } else if (kind == 'A') {
      std::vector<uint32_t> table((size_t)PPK_SKETCH_COUNT_ROWS << t_bits, 0);
      for (uint64_t h : hashes)
        for (int r = 0; r < PPK_SKETCH_COUNT_ROWS; ++r) ++table[((size_t)r << t_bits) + ppk_sketch_count_index(h, r, t_bits)];
      for (size_t i = 0; i < hashes.size(); ++i) {
        int want = 0;
        ls >> want;
        bool ok = true;
        for (int r = 0; r < PPK_SKETCH_COUNT_ROWS; ++r)
          ok = ok && table[((size_t)r << t_bits) + ppk_sketch_count_index(hashes[i], r, t_bits)] >= t_min;
        CHECK((int)ok == want, "hash %zu of a table of %d bits: admitted %d, model %d", i, t_bits, (int)ok, want);
      }
    }
  }
  std::printf("%llu checks, %d wrong\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}

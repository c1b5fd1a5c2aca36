// Host-side check of the sketch rule in poppunk_amd/csrc/ppk_device.h (hash, its rolling form, bin, densify) against
// values written by tests/sketch_model.py: built and run by test_sketch_host.py (host only, under the
// undefined-behaviour and address sanitizers).  argv[1]: a text file of records
//   S <k> <strand_preserved> <nbins> <codes as digits>   a sequence; then one line per valid k-mer, in order:
//   V <start> <hash, hex> <bin>
//   E                                                    ends the sequence
//   B <hash, hex> <nbins> <bin>                          one bin on its own
//   K <hash, hex> <kept, hex>                            what a bin keeps of a hash
//   M <nbins> <non-empty bins ...>                       a state before densification; then
//   R <source bin of every bin ...>
// Exit status 0 and the count of checks on stdout, or the first failures on stderr and exit status 1.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
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

struct Kmer {
  long long start;
  uint64_t h;
  uint32_t bin;
};

// every valid k-mer of `codes`, hashed from the definition
static std::vector<Kmer> direct(const std::vector<uint8_t> &codes, int k, int sp, uint32_t nbins) {
  std::vector<Kmer> out;
  for (long long i = 0; i + k <= (long long)codes.size(); ++i) {
    bool ok = true;
    for (int j = 0; j < k; ++j) ok = ok && codes[(size_t)(i + j)] < 4;
    if (!ok) continue;
    const uint64_t h = ppk_sketch_hash(codes.data() + i, k, sp);
    out.push_back({i, h, ppk_sketch_bin(h, nbins)});
  }
  return out;
}

// ... and the way a lane of the kernel takes them: runs of `piece` start positions, each warmed up over k - 1 codes
static std::vector<Kmer> rolled(const std::vector<uint8_t> &codes, int k, int sp, uint32_t nbins, long long piece) {
  std::vector<Kmer> out;
  uint64_t terms[5][4];
  for (unsigned c = 0; c < 5; ++c) ppk_sketch_terms(c, k, terms[c]);
  const long long n_start = (long long)codes.size() - k + 1;
  for (long long q0 = 0; q0 < n_start; q0 += piece) {
    const long long q1 = q0 + piece < n_start ? q0 + piece : n_start;
    uint64_t f = 0, r = 0;
    int run = 0;
    for (int t = 0; t < k - 1; ++t) {
      const unsigned c = codes[(size_t)(q0 + t)] < 4 ? codes[(size_t)(q0 + t)] : 4;
      ppk_sketch_roll(f, r, terms[c][0], terms[c][1], 0, 0);
      run = c < 4 ? run + 1 : 0;
    }
    unsigned o = 4;
    for (long long q = q0; q < q1; ++q) {
      const unsigned c = codes[(size_t)(q + k - 1)] < 4 ? codes[(size_t)(q + k - 1)] : 4;
      ppk_sketch_roll(f, r, terms[c][0], terms[c][1], terms[o][2], terms[o][3]);
      run = c < 4 ? run + 1 : 0;
      if (run >= k) {
        const uint64_t h = ppk_sketch_pick(f, r, sp);
        out.push_back({q, h, ppk_sketch_bin(h, nbins)});
      }
      o = codes[(size_t)q] < 4 ? codes[(size_t)q] : 4;
    }
  }
  return out;
}

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
  std::vector<Kmer> want, got;
  std::vector<uint8_t> codes;
  std::vector<uint32_t> full;
  int k = 0, sp = 0;
  uint32_t nbins = 0;
  size_t at = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    char kind = 0;
    ls >> kind;
    if (kind == 'S') {
      std::string digits;
      ls >> k >> sp >> nbins >> digits;
      codes.clear();
      for (char c : digits) codes.push_back((uint8_t)(c - '0'));
      got = direct(codes, k, sp, nbins);
      for (long long piece : {1ll, 7ll, 128ll}) {
        const std::vector<Kmer> again = rolled(codes, k, sp, nbins, piece);
        CHECK(again.size() == got.size(), "k %d piece %lld: %zu k-mers rolled, %zu direct", k, piece, again.size(), got.size());
        for (size_t i = 0; i < again.size() && i < got.size(); ++i)
          CHECK(again[i].start == got[i].start && again[i].h == got[i].h && again[i].bin == got[i].bin,
                "k %d piece %lld, k-mer %zu: rolled %lld %016" PRIx64 ", direct %lld %016" PRIx64, k, piece, i,
                again[i].start, again[i].h, got[i].start, got[i].h);
      }
      at = 0;
    } else if (kind == 'V') {
      Kmer w{};
      ls >> w.start >> std::hex >> w.h >> std::dec >> w.bin;
      CHECK(at < got.size() && got[at].start == w.start && got[at].h == w.h && got[at].bin == w.bin,
            "k %d, k-mer %zu: model %lld %016" PRIx64 " bin %u", k, at, w.start, w.h, w.bin);
      CHECK(w.bin < nbins, "bin %u of %u", w.bin, nbins);
      ++at;
    } else if (kind == 'E') {
      CHECK(at == got.size(), "k %d: the model lists %zu k-mers, the helpers find %zu", k, at, got.size());
    } else if (kind == 'B') {
      uint64_t h = 0;
      uint32_t nb = 0, bin = 0;
      ls >> std::hex >> h >> std::dec >> nb >> bin;
      CHECK(ppk_sketch_bin(h, nb) == bin && bin < nb, "bin of %016" PRIx64 " in %u: %u, model %u", h, nb, ppk_sketch_bin(h, nb), bin);
    } else if (kind == 'K') {
      uint64_t h = 0, kept = 0;
      ls >> std::hex >> h >> kept;
      CHECK(ppk_sketch_keep(h) == kept, "kept of %016" PRIx64, h);
    } else if (kind == 'M') {
      ls >> nbins;
      full.clear();
      uint32_t b;
      while (ls >> b) full.push_back(b);
    } else if (kind == 'R') {
      // the block masks, and per block the first non-empty bin of the blocks after it, cyclically, as the kernel's
      // finish pass hands them to the helper
      const uint32_t blocks = nbins / 64;
      std::vector<uint64_t> mask(blocks, 0);
      for (uint32_t b : full) mask[b / 64] |= (uint64_t)1 << (b % 64);
      for (uint32_t bin = 0; bin < nbins; ++bin) {
        uint32_t src = 0;
        ls >> src;
        const uint32_t blk = bin / 64;
        uint32_t next = 0;
        for (uint32_t d = 1; d <= blocks; ++d) {
          const uint32_t other = (blk + d) % blocks;
          if (mask[other]) {
            next = other * 64 + (uint32_t)__builtin_ctzll(mask[other]);
            break;
          }
        }
        const uint32_t mine = ppk_sketch_densify_src(mask[blk], bin % 64, blk, next);
        CHECK(mine == src, "densify: bin %u takes %u, model %u", bin, mine, src);
      }
    }
  }
  std::printf("%llu checks, %d wrong\n", g_checks, g_bad);
  return g_bad ? 1 : 0;
}

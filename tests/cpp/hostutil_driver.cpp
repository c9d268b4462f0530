// hostutil_driver.cpp -- the pure host helpers of the host-pointer entries (csrc/msa_hostutil.h) on the CPU, built
// with -fsanitize=address,undefined: every expected value is written out here.  Prints "OK" and exits 0, or names
// the first check that failed and exits 1.
#include <cstdio>
#include <string>
#include <vector>

#include "msa_hostutil.h"

using namespace msa_host;

static int failures = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      failures++;                                                 \
    }                                                             \
  } while (0)

static std::string cigar(const std::string& ops) { return cigar_of(ops.data(), ops.size()); }

static std::string completed(std::string ops, int64_t i, int64_t j, Border rule, int64_t* ret = nullptr) {
  const int64_t r = complete_border(ops, i, j, rule);
  if (ret) *ret = r;
  return ops;
}

// symbols 0 .. n-1 of "abcdefghi"
static int encode_first(SymbolMap& map, int n, uint8_t* out) { return map.encode("abcdefghi", (size_t)n, out); }

int main() {
  // cigar_of: ops end -> start, the string start -> end
  CHECK(cigar("") == "");
  CHECK(cigar_of(nullptr, 0) == "");
  CHECK(cigar("M") == "1M");
  CHECK(cigar("MMMMM") == "5M");
  CHECK(cigar("MID") == "1D1I1M");
  CHECK(cigar("MDMDM") == "1M1D1M1D1M");
  CHECK(cigar("MMDIIIM") == "1M3I1D2M");
  CHECK(cigar(std::string(12, 'D') + std::string(100, 'M')) == "100M12D");

  // complete_border: the walk stopped at (i, j)
  int64_t j = -1;
  CHECK(completed("MM", 3, 0, BORDER_GLOBAL, &j) == "MMIII" && j == 0);
  CHECK(completed("MM", 0, 2, BORDER_GLOBAL, &j) == "MMDD" && j == 2);
  CHECK(completed("MM", 0, 0, BORDER_GLOBAL, &j) == "MM" && j == 0);
  CHECK(completed("", 4, 0, BORDER_GLOBAL) == "IIII");
  CHECK(completed("MM", 3, 0, BORDER_FIT, &j) == "MMIII" && j == 0);
  CHECK(completed("MM", 0, 2, BORDER_FIT, &j) == "MM" && j == 2);  // the symbols before column 2 are free
  CHECK(completed("MM", 0, 0, BORDER_FIT, &j) == "MM" && j == 0);
  CHECK(completed("MM", 3, 0, BORDER_NONE) == "MM");
  CHECK(completed("MM", 0, 2, BORDER_NONE) == "MM");

  // SymbolMap: first-seen codes up to the limit
  uint8_t out[16];
  {
    SymbolMap m8(8);
    CHECK(encode_first(m8, 8, out) == MSA_OK && out[0] == 0 && out[7] == 7 && m8.size() == 8);
    CHECK(encode_first(m8, 9, out) == MSA_ERR_ALPHABET);
    CHECK(m8.encode("hgah", 4, out) == MSA_OK && out[0] == 7 && out[1] == 6 && out[2] == 0 && out[3] == 7);
    SymbolMap m7(7);
    CHECK(encode_first(m7, 7, out) == MSA_OK && out[6] == 6);
    CHECK(encode_first(m7, 8, out) == MSA_ERR_ALPHABET);
  }
  {  // a preset holds the first codes whether its symbols occur or not
    SymbolMap dna(8, "ACGT");
    CHECK(dna.size() == 4);
    CHECK(dna.encode("TNGCA", 5, out) == MSA_OK);
    CHECK(out[0] == 3 && out[1] == 4 && out[2] == 2 && out[3] == 1 && out[4] == 0);
    CHECK(dna.encode("RYK", 3, out) == MSA_OK && out[2] == 7);
    CHECK(dna.encode("W", 1, out) == MSA_ERR_ALPHABET);
    SymbolMap dna7(7, "ACGT");
    CHECK(dna7.encode("NRY", 3, out) == MSA_OK && out[2] == 6);
    CHECK(dna7.encode("K", 1, out) == MSA_ERR_ALPHABET);
  }
  {  // a fixed map: the alphabet's symbols and no other; a duplicate is refused
    SymbolMap fx(8);
    CHECK(fx.add('x') && fx.add('y') && !fx.add('x') && fx.add('z'));
    fx.fix();
    CHECK(fx.size() == 3 && !fx.add('w'));
    CHECK(fx.encode("zyxz", 4, out) == MSA_OK && out[0] == 2 && out[1] == 1 && out[2] == 0 && out[3] == 2);
    CHECK(fx.encode("xyw", 3, out) == MSA_ERR_ALPHABET);
    SymbolMap full(8);
    for (int k = 0; k < 8; ++k) CHECK(full.add((char)('a' + k)));
    CHECK(!full.add('i'));
  }
  {  // every byte value is a symbol: 0 and 255 too
    SymbolMap m(8);
    const char s[4] = {'\0', '\xff', '\0', '\x80'};
    CHECK(m.encode(s, 4, out) == MSA_OK && out[0] == 0 && out[1] == 1 && out[2] == 0 && out[3] == 2);
    SymbolMap fx(8);
    CHECK(fx.add('\xff') && fx.add('\0'));
    fx.fix();
    CHECK(fx.encode(s, 3, out) == MSA_OK && out[0] == 1 && out[1] == 0 && out[2] == 1);
    CHECK(fx.encode(s, 4, out) == MSA_ERR_ALPHABET);
  }
  CHECK(SymbolMap(8).encode("", 0, nullptr) == MSA_OK);

  // ops_offsets: the vector tests/test_host.py::test_ops_layout pins for Plan.ops_layout
  {
    const int64_t m[2] = {1, 63}, n[2] = {1, 70};
    CHECK((ops_offsets(m, n, 2) == std::vector<int64_t>{0, 16, 160}));
    CHECK((ops_offsets(m, n, 0) == std::vector<int64_t>{0}));
    const int64_t m14 = 7, n14 = 7;  // m + n + 2 = 16: no padding
    CHECK((ops_offsets(&m14, &n14, 1) == std::vector<int64_t>{0, 16}));
  }

  // SinglePairDesc: one pair, its arrays alive with it
  {
    SinglePairDesc sd(MSA_REF_GOTOH, MSA_CELLS_DIR, 5, 9);
    CHECK(sd.d.alg == MSA_REF_GOTOH && sd.d.cells == MSA_CELLS_DIR && sd.d.single == 1 && sd.d.n_pairs == 1);
    CHECK(sd.d.band == -1 && sd.d.match == 0 && sd.d.track_end == 0);
    CHECK(*sd.d.m == 5 && *sd.d.n == 9 && *sd.d.a_off == 0 && *sd.d.b_off == 0);
  }

  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}

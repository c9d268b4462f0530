// refwalk_driver.cpp -- the reference API's pure host rules (csrc/msa_refwalk.h) on the CPU, built with
// -fsanitize=address,undefined and linking nothing of the product.  "selftest" checks what has hand-written
// expected values (written out here); the other commands print what the header computes from the caller's tables,
// ops, paths or keys, for tests/test_host.py to compare with the fixtures and the oracle.  One command per case on
// stdin, whitespace-separated; each answer ends with END_CASE.
//   selftest
//   walk i|d m n idA idB end_type g h A B  <3 (m+1)(n+1) cells: T1, T2, T3 row-major>    find_alignment
//   ops m n idA idB end_i end_j end_t OPS|-                                               nodes_from_ops
//   order num fix                                                                         solve_order
//   text n_solved m n A B k  <k x: i j t>                                                 alignment_text
//   part m n p  <2 (p+1) keys>                                                            partition_from_keys
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "msa_refwalk.h"

using namespace msa_host;

static int failures = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      failures++;                                                 \
    }                                                             \
  } while (0)

static bool same(const msa_node& a, uint64_t i, uint64_t j, int t) { return a.i == i && a.j == j && a.t == t; }

static void print_nodes(const std::vector<msa_node>& v) {
  std::printf("NODES %zu\n", v.size());
  for (const msa_node& x : v) std::printf("%llu %llu %d\n", (unsigned long long)x.i, (unsigned long long)x.j, x.t);
}

static std::vector<SubResult> subs(std::initializer_list<int> lens) {
  std::vector<SubResult> s;
  for (int len : lens) {  // len < 0: not solved; node k of subproblem q is (q, k, 1)
    SubResult r;
    r.solved = len >= 0;
    for (int k = 0; k < len; ++k) r.nodes.push_back(msa_node{s.size(), (uint64_t)k, 1, 0});
    s.push_back(r);
  }
  return s;
}
static std::string firsts(const std::vector<msa_node>& v) {
  std::string s;
  for (const msa_node& x : v) s += (char)('0' + x.i);
  return s;
}

static void selftest() {
  // solve_order (main_alignment.cpp:232-341): up to 3 subproblems only the first; then three rounds r, r+3, ...
  using V = std::vector<size_t>;
  CHECK((solve_order(1, false) == V{0}));
  CHECK((solve_order(2, false) == V{0}));
  CHECK((solve_order(3, false) == V{0}));
  CHECK((solve_order(4, false) == V{0, 3, 1, 2}));
  CHECK((solve_order(5, false) == V{0, 3, 1, 4, 2}));
  CHECK((solve_order(6, false) == V{0, 3, 1, 4, 2, 5}));
  CHECK((solve_order(7, false) == V{0, 3, 6, 1, 4, 2, 5}));
  CHECK((solve_order(8, false) == V{0, 3, 6, 1, 4, 7, 2, 5}));
  for (size_t num = 1; num <= 8; ++num) {
    V all;
    for (size_t k = 0; k < num; ++k) all.push_back(k);
    CHECK(solve_order(num, true) == all);
  }

  // stitch (:344-348): links 1 .. num-2 only, an unsolved or empty subproblem ends the list
  CHECK(firsts(stitch(subs({2}), false)) == "00");
  CHECK(firsts(stitch(subs({2, 1}), false)) == "00");          // the link into the last is never made
  CHECK(firsts(stitch(subs({2, 1}), true)) == "001");
  CHECK(firsts(stitch(subs({1, 2, 1, 3}), false)) == "0112");
  CHECK(firsts(stitch(subs({1, 2, 1, 3}), true)) == "0112333");
  CHECK(firsts(stitch(subs({1, -1, 1, 3}), false)) == "0");    // subproblem 1 not solved
  CHECK(firsts(stitch(subs({1, 0, 1, 3}), true)) == "0");      // alignment_begin == NULL
  CHECK(firsts(stitch(subs({0, 2}), true)) == "");

  // the end-node rule (:112-146)
  const double fin[3] = {3, 4, 4};
  CHECK(same(end_node_of(1, 2, fin, 5, 7, 2, 1), 7, 8, 1));
  CHECK(same(end_node_of(2, 2, fin, 5, 7, 2, 1), 0, 8, 2));
  CHECK(same(end_node_of(3, 2, fin, 5, 7, 2, 1), 7, 0, 3));
  CHECK(same(end_node_of(-1, 2, fin, 5, 7, 2, 1), 0, 8, 2));   // T2 = T3 > T1: T2
  CHECK(same(end_node_of(-3, 2, fin, 5, 7, 2, 1), 7, 0, 3));   // h_prime on T3
  const double fin1[3] = {6, 4, 4};
  CHECK(same(end_node_of(-2, 2, fin1, 5, 7, 2, 1), 7, 8, 1));  // 6 >= 4 + 2: ties go to T1
  CHECK(same(end_node_of(-2, 2.5, fin1, 5, 7, 2, 1), 0, 8, 2));
  const double ninf[3] = {-INFINITY, -INFINITY, -INFINITY};
  CHECK(same(end_node_of(-1, 2, ninf, 0, 4, 0, 0), 0, 4, 1));
  CHECK(dinf(MSA_NEG) == -INFINITY && dinf(-7) == -7.0 && dinf(INT32_MIN) == (double)INT32_MIN);

  // the table borders
  const int32_t N = MSA_NEG, M = INT32_MIN;
  int32_t v[3];
  auto is = [&](int32_t a, int32_t b, int32_t c) { return v[0] == a && v[1] == b && v[2] == c; };
  ref_row0(-1, 1, 2, 0, v); CHECK(is(0, N, N));
  ref_row0(-1, 1, 2, 3, v); CHECK(is(N, -5, N));
  ref_row0(-2, 1, 2, 0, v); CHECK(is(N, 0, N));
  ref_row0(-2, 1, 2, 3, v); CHECK(is(N, -3, N));
  ref_row0(-3, 1, 2, 0, v); CHECK(is(N, N, 0));
  ref_row0(1, 1, 2, 0, v); CHECK(is(0, N, N));
  ref_row0(1, 1, 2, 2, v); CHECK(is(N, N, N));
  ref_row0(3, 1, 2, 2, v); CHECK(is(N, N, N));
  ref_row0(2, 1, 2, 0, v); CHECK(is(N, N, N));
  ref_row0(2, 1, 2, 2, v); CHECK(is(N, -4, N));
  part_row0(1, 3, 0, v); CHECK(is(0, M, M));
  part_row0(1, 3, 2, v); CHECK(is(M, M, M));
  part_row0(2, 3, 0, v); CHECK(is(M, M, M));
  part_row0(2, 3, 2, v); CHECK(is(M, -6, M));
  part_row0(-1, 3, 0, v); CHECK(is(M, M, M));

  // which g, h the int32 kernels take
  CHECK(exact_gh(1, 2) && exact_gh(0, 0) && exact_gh(3, -2) && exact_gh(1048575, 0));
  CHECK(!exact_gh(0.5, 1) && !exact_gh(1, 0.25) && !exact_gh(-1, 2) && !exact_gh(1, -2));
  CHECK(!exact_gh(1048576, 0) && !exact_gh(NAN, 1) && !exact_gh(1, INFINITY));

  // partition_from_keys' key decoding: value (biased) << 32 | ~index (30 bits) << 2 | type.  m = 10, n = 8, p = 2:
  // bands of 5 rows and 4 columns; row winner at index 1 * 8 + 2 -> (5 + 1, 1 + 2), column winner at index
  // 1 * 10 + 3 -> (1 + 3, 4 + 1); ties go to the column
  auto key = [](int32_t val, uint32_t idx, int t) {
    return ((unsigned long long)((uint32_t)val ^ 0x80000000u) << 32) | ((unsigned long long)(~idx & 0x3fffffffu) << 2) |
           (unsigned long long)t;
  };
  std::vector<unsigned long long> hk = {0, 0, key(7, 10, 2), key(7, 13, 1), 0, 0};
  std::vector<msa_node> part = partition_from_keys(hk, 10, 8, 2);
  CHECK(part.size() == 3 && same(part[0], 0, 0, -1) && same(part[1], 4, 5, 1) && same(part[2], 10, 8, 1));
  hk[2] = key(8, 10, 2);
  part = partition_from_keys(hk, 10, 8, 2);
  CHECK(part.size() == 3 && same(part[1], 6, 3, 2));
  hk[2] = key(-3, 10, 3);
  hk[3] = 0;  // no column cell: the row's -3 beats INT_MIN
  part = partition_from_keys(hk, 10, 8, 2);
  CHECK(part.size() == 3 && same(part[1], 6, 3, 3));
  part = partition_from_keys({0, 0, 0, 0}, 10, 8, 1);
  CHECK(part.size() == 2 && same(part[0], 0, 0, -1) && same(part[1], 10, 8, 1));

  std::puts(failures ? "SELFTEST FAILED" : "SELFTEST OK");
}

template <class T>
static void walk(std::istream& in, T (*parse)(const std::string&)) {
  int64_t m, n;
  uint64_t idA, idB;
  int end_type;
  std::string gs, hs, A, B, tok;
  in >> m >> n >> idA >> idB >> end_type >> gs >> hs >> A >> B;
  const double g = std::strtod(gs.c_str(), nullptr), h = std::strtod(hs.c_str(), nullptr);
  const size_t cells = (size_t)((m + 1) * (n + 1));
  std::vector<T> tab[3];
  for (auto& t : tab)
    for (size_t e = 0; e < cells && (in >> tok); ++e) t.push_back(parse(tok));
  if (tab[2].size() != cells || A.size() < idA + (uint64_t)m || B.size() < idB + (uint64_t)n) {
    std::printf("ERROR bad walk case\n");
    return;
  }
  // exactly the caller's symbols; f (subproblem_alignment.h:83-88) compares the 1-based A[id_A + i], B[id_B + j]
  const std::vector<char> A1(A.begin(), A.end()), B1(B.begin(), B.end());
  auto f = [&](int64_t i, int64_t j) { return A1[idA + (uint64_t)i - 1] == B1[idB + (uint64_t)j - 1]; };
  std::vector<msa_node> nodes;
  msa_node endn{};
  const int rc = find_alignment(tab[0].data(), tab[1].data(), tab[2].data(), m, n, idA, idB, end_type, g, h, f,
                                nodes, endn);
  std::printf("RC %d\n", rc);
  if (rc != MSA_OK) return;
  std::printf("END %llu %llu %d\n", (unsigned long long)endn.i, (unsigned long long)endn.j, endn.t);
  print_nodes(nodes);
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "selftest") {
      selftest();
    } else if (cmd == "walk") {
      std::string kind;
      std::cin >> kind;
      if (kind == "i")
        walk<int32_t>(std::cin, [](const std::string& s) { return (int32_t)std::strtol(s.c_str(), nullptr, 10); });
      else
        walk<double>(std::cin, [](const std::string& s) { return std::strtod(s.c_str(), nullptr); });
    } else if (cmd == "ops") {
      int64_t m, n;
      uint64_t idA, idB;
      msa_node endn{};
      std::string s;
      std::cin >> m >> n >> idA >> idB >> endn.i >> endn.j >> endn.t >> s;
      const std::vector<char> ops(s == "-" ? s.end() : s.begin(), s.end());  // exactly the ops: a read past them shows
      std::vector<msa_node> nodes;
      const int rc = nodes_from_ops(ops.data(), ops.size(), m, n, idA, idB, endn, nodes);
      std::printf("RC %d\n", rc);
      if (rc == MSA_OK) print_nodes(nodes);
    } else if (cmd == "order") {
      size_t num;
      int fix;
      std::cin >> num >> fix;
      std::printf("ORDER");
      for (size_t k : solve_order(num, fix != 0)) std::printf(" %zu", k);
      std::printf("\n");
    } else if (cmd == "text") {
      size_t n_solved, m, n, k;
      std::string A, B;
      std::cin >> n_solved >> m >> n >> A >> B >> k;
      std::vector<msa_node> path(k);
      for (msa_node& x : path) std::cin >> x.i >> x.j >> x.t;
      // the caller's 1-based arrays, slot 0 unused, exactly m + 1 and n + 1 long
      std::vector<char> A1(1, '\0'), B1(1, '\0');
      A1.insert(A1.end(), A.begin(), A.end());
      B1.insert(B1.end(), B.begin(), B.end());
      if (A.size() != m || B.size() != n) {
        std::printf("ERROR bad text case\n");
      } else {
        const std::string s = alignment_text(n_solved, path, A1.data(), m, B1.data(), n);
        std::fwrite(s.data(), 1, s.size(), stdout);
      }
    } else if (cmd == "part") {
      int64_t m, n;
      size_t p;
      std::cin >> m >> n >> p;
      std::vector<unsigned long long> hk(2 * (p + 1));
      for (auto& x : hk) std::cin >> x;
      print_nodes(partition_from_keys(hk, m, n, p));
    } else {
      std::printf("ERROR unknown command %s\n", cmd.c_str());
      return 2;
    }
    std::printf("END_CASE\n");
  }
  return failures ? 1 : 0;
}

// msa_refwalk.h -- the pure host-side rules of the reference's API (msa_refapi.inc): Subproblem::find_alignment
// (subproblem_alignment.cpp:105-172, quirks kept), the table borders, optimal_alignment's solve order, stitching
// and stdout text (main_alignment.cpp), partial.cpp's partition tail.  Standard C++ only -- no HIP -- so that
// tests/cpp/refwalk_driver.cpp runs every one of them on the CPU under sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "msa.h"

#ifndef MSA_NEG
#define MSA_NEG (-(1 << 30))  // -inf of the int32 tables (msa_kernels.hip)
#endif

namespace msa_host {

inline bool integral_small(double x) {
  return std::isfinite(x) && std::floor(x) == x && std::fabs(x) < (double)(1 << 20);
}
// g, h the int32 kernels hold exactly; any other pair takes the double row sweep
inline bool exact_gh(double g, double h) { return integral_small(g) && integral_small(h) && g >= 0 && g + h >= 0; }

// A table cell as the reference's double: int32 tables hold MSA_NEG for -inf.
inline double dinf(int32_t x) { return x == MSA_NEG ? -INFINITY : (double)x; }
inline double cell(int32_t x) { return dinf(x); }
inline double cell(double x) { return x; }

// Row 0 of the reference Gotoh tables (ComputeFirstRowMapThread, :212-227).
inline void ref_row0(int st, int g, int h, int64_t c, int32_t v[3]) {
  const int32_t NEG = MSA_NEG;
  if (c == 0) {
    v[0] = (st == 1 || st == -1) ? 0 : NEG;
    v[1] = (st == -2) ? 0 : NEG;
    v[2] = (st == -3) ? 0 : NEG;
  } else {
    v[0] = NEG;
    v[2] = NEG;
    v[1] = (st == -2) ? (int32_t)(-g * c) : ((st == 1 || st == 3) ? NEG : (int32_t)(-h - g * c));
  }
}

// Row 0 of partial.cpp's int tables (initializeTables, :13-31).
inline void part_row0(int st, int GH, int64_t c, int32_t v[3]) {
  v[0] = (c == 0 && st == 1) ? 0 : INT32_MIN;
  v[1] = (c >= 1 && st == 2) ? (int32_t)((uint32_t)(-GH) * (uint32_t)c) : INT32_MIN;
  v[2] = INT32_MIN;
}

// ---- Subproblem::find_alignment (subproblem_alignment.cpp:105-172) ----------------------------------------------
// A walk is the tables it visits, end -> start, one op per step: the table the step leaves ('M' T1, 'D' T2, 'I' T3)
// -- what the device walk writes (msa_plan_traceback_gotoh) and what table_ops below makes of host tables.
// nodes_from_ops turns either into the reference's align nodes.

// The table a node of type t walks in: find_alignment's else branches take every type but 1 and 2 as T3.
inline int table_of(int t) { return (t == 1 || t == 2) ? t : 3; }

// The node of type t at cell (i, j): a T2 node has i = 0, a T3 node j = 0, the rest is offset by the window's origin.
inline msa_node node_at(int t, int64_t i, int64_t j, uint64_t idA, uint64_t idB) {
  return msa_node{table_of(t) == 2 ? 0 : (uint64_t)i + idA, table_of(t) == 3 ? 0 : (uint64_t)j + idB, t, 0};
}

// One step back from (i, j) out of table ct: T1 goes diagonally, T2 along the row, T3 along the column.
inline void step_back(int ct, int64_t& i, int64_t& j) {
  if (ct != 2) i--;
  if (ct != 3) j--;
}

// alignment_end (:112-146) from fin = (T1, T2, T3)(m, n): end_type > 0 names its type, otherwise the best of the
// three with h_prime added to the table end_type <= -2 names; ties go to T1, then T2.
inline msa_node end_node_of(int end_type, double h, const double fin[3], int64_t m, int64_t n, uint64_t idA,
                            uint64_t idB) {
  int t = end_type;
  if (end_type <= 0) {
    const double t1 = fin[0], t2 = fin[1] + (end_type == -2 ? h : 0.0), t3 = fin[2] + (end_type == -3 ? h : 0.0);
    t = (t1 >= t2 && t1 >= t3) ? 1 : ((t2 >= t1 && t2 >= t3) ? 2 : 3);
  }
  return node_at(t, m, n, idA, idB);
}

// The walk (:147-169) over row-major (m + 1) x (n + 1) tables of int32 (MSA_NEG = -inf) or double, from (m, n) in
// the table of a type-t_end node until row or column 0.  Each step takes the first of T1, T2, T3 whose cell the
// reference's own double expression reproduces: f + T out of T1; -g + T within T2 or T3 and -g - h + T into them,
// in that evaluation order (it matters for non-integral g, h).  f(i, j): do the symbols of cell (i, j) match.
// MSA_ERR_NOMATCH: no table does -- the reference would loop forever on an uninitialised node there.
template <class T, class F>
int table_ops(const T* T1, const T* T2, const T* T3, int64_t m, int64_t n, int t_end, double g, double h, F f,
              std::vector<char>& ops) {
  const T* const tabs[3] = {T1, T2, T3};
  auto at = [&](int t, int64_t i, int64_t j) { return cell(tabs[t - 1][i * (n + 1) + j]); };
  ops.clear();
  int ct = table_of(t_end);
  for (int64_t i = m, j = n; i > 0 && j > 0;) {
    ops.push_back("MDI"[ct - 1]);
    const double v = at(ct, i, j), fij = ct == 1 ? (f(i, j) ? 1.0 : 0.0) : 0.0;
    step_back(ct, i, j);
    int nt = 0;
    for (int t = 1; t <= 3 && !nt; ++t) {
      const double p = at(t, i, j);
      if (v == (ct == 1 ? fij + p : (t == ct ? -g + p : -g - h + p))) nt = t;
    }
    if (!nt) return MSA_ERR_NOMATCH;
    ct = nt;
  }
  return MSA_OK;
}

// The align nodes, alignment_begin .. alignment_end, of a walk from (m, n) whose end node is endn.  Op 0 belongs to
// endn; the node of op k >= 1 is created by step k - 1, with the type of the table it enters, at the cell it enters
// -- but a T1 -> T1 step offsets j by id_A (quirk Q2, the typo of :151, kept).  The node the last step would
// create has no op: alignment_begin = curr_point->next drops it (quirk Q1, :170).  MSA_ERR_NOMATCH: ops that are
// no such walk.
inline int nodes_from_ops(const char* ops, size_t n_ops, int64_t m, int64_t n, uint64_t idA, uint64_t idB,
                          const msa_node& endn, std::vector<msa_node>& nodes) {
  nodes.clear();
  nodes.reserve(n_ops);
  int64_t i = m, j = n;
  int prev = 0;
  for (size_t k = 0; k < n_ops; ++k) {
    const int ct = ops[k] == 'M' ? 1 : (ops[k] == 'D' ? 2 : (ops[k] == 'I' ? 3 : 0));
    if (!ct || (k == 0 && ct != table_of(endn.t))) return MSA_ERR_NOMATCH;  // no table, or not the end node's
    if (i <= 0 || j <= 0) return MSA_ERR_NOMATCH;                            // past find_alignment's stop
    nodes.push_back(k == 0 ? endn : node_at(ct, i, j, idA, (prev == 1 && ct == 1) ? idA : idB));  // Q2
    step_back(ct, i, j);
    prev = ct;
  }
  if (i != 0 && j != 0) return MSA_ERR_NOMATCH;  // stopped before the border (no ops at all included)
  std::reverse(nodes.begin(), nodes.end());
  return MSA_OK;
}

// find_alignment over host tables: the end node, the walk, its nodes.
template <class T, class F>
int find_alignment(const T* T1, const T* T2, const T* T3, int64_t m, int64_t n, uint64_t idA, uint64_t idB,
                   int end_type, double g, double h, F f, std::vector<msa_node>& nodes, msa_node& endn) {
  const int64_t e = m * (n + 1) + n;
  const double fin[3] = {cell(T1[e]), cell(T2[e]), cell(T3[e])};
  endn = end_node_of(end_type, h, fin, m, n, idA, idB);
  std::vector<char> ops;
  const int rc = table_ops(T1, T2, T3, m, n, endn.t, g, h, f, ops);
  return rc != MSA_OK ? rc : nodes_from_ops(ops.data(), ops.size(), m, n, idA, idB, endn, nodes);
}

// ---- optimal_alignment (main_alignment.cpp:158-351) -------------------------------------------------------------

// One solved subproblem: its node list (alignment_begin .. alignment_end, possibly empty: alignment_begin = NULL)
// and its alignment_end node.
struct SubResult {
  bool solved = false;
  std::vector<msa_node> nodes;
  msa_node endn{};
};

// Which subproblems optimal_alignment solves, in its order (main_alignment.cpp:232-341):
// round r = 0, 1, 2 takes r, r+3, ... while i < num-3 (threads) and then one more
// at the first i past that, if i < num.  Rounds 1 and 2 run only when num > 3, so
// with 2 or 3 subproblems only subproblem 0 is solved.  fix: every subproblem.
inline std::vector<size_t> solve_order(size_t num, bool fix) {
  std::vector<size_t> order;
  if (fix) {
    for (size_t k = 0; k < num; ++k) order.push_back(k);
    return order;
  }
  const bool num_sub_3 = num > 3;
  for (size_t r = 0; r < 3; ++r) {
    if (r > 0 && !num_sub_3) break;
    size_t i = r;
    while (num_sub_3 && i < num - 3) {
      order.push_back(i);
      i += 3;
    }
    if (i < num) order.push_back(i);
  }
  return order;
}

// The stitched list (:344-348): end of subproblem i-1 -> begin of subproblem i for i = 1 .. num-2; the link into
// the last subproblem is never made (fix: made).
inline std::vector<msa_node> stitch(const std::vector<SubResult>& sub, bool fix) {
  const size_t num = sub.size();
  std::vector<msa_node> out;
  const size_t last_link = fix ? num - 1 : (num >= 2 ? num - 2 : 0);
  for (size_t k = 0; k < num; ++k) {
    if (!sub[k].solved || sub[k].nodes.empty()) break;  // alignment_begin == NULL ends the walk
    out.insert(out.end(), sub[k].nodes.begin(), sub[k].nodes.end());
    if (k + 1 > last_link || k + 1 >= num) break;  // the end node's next stays NULL
  }
  return out;
}

// stdout of main_alignment_function / optimal_alignment: bp1..bp4 once per solved subproblem (the reference's
// threads interleave these lines), then print_seq (main_alignment.cpp:32-55) of the node list on the caller's
// UNSWAPPED 1-based arrays (quirk Q3); indices past the caller's buffers print '?' (the reference reads out of
// bounds).
inline std::string alignment_text(size_t n_solved, const std::vector<msa_node>& path, const char* A1, size_t m,
                                  const char* B1, size_t n) {
  static const char hdr[] = "bp1\nbp1.2\nbp2\nbp3\nbp4\n";
  const size_t H = sizeof(hdr) - 1, L = path.size();
  std::string s(H * n_solved + 2 * (L + 1), '\n');  // (the two line ends are in place)
  char* o = &s[0];
  for (size_t k = 0; k < n_solved; ++k, o += H) std::memcpy(o, hdr, H);
  for (size_t k = 0; k < L; ++k)
    o[k] = (path[k].t == 1 || path[k].t == 3) ? (path[k].i <= m ? A1[path[k].i] : '?') : '-';
  o += L + 1;
  for (size_t k = 0; k < L; ++k)
    o[k] = (path[k].t == 1 || path[k].t == 2) ? (path[k].j <= n ? B1[path[k].j] : '?') : '-';
  return s;
}

// ---- partial.cpp ------------------------------------------------------------------------------------------------

// findPartitionParallel's tail (partial.cpp:128-145) from the band winners partition_kernel
// reduced: per k the row band's or the column band's best cell, then (0,0,-1), (m,n,1) and
// the reference's std::sort.
inline std::vector<msa_node> partition_from_keys(const std::vector<unsigned long long>& hk, int64_t m, int64_t n,
                                                 size_t p) {
  const int64_t bm = m / (int64_t)p, bn = n / (int64_t)p;
  std::vector<msa_node> part;
  part.push_back(msa_node{0, 0, -1, 0});
  for (size_t k = 1; k < p; ++k) {
    // decode a band winner; key 0 = no cell beat INT_MIN -> {0,0,0}
    auto decode = [&](unsigned long long key, bool row, int32_t& val, msa_node& nd) {
      nd = msa_node{0, 0, 0, 0};
      val = INT32_MIN;
      if (!key) return;
      val = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
      const int64_t idx = (int64_t)((~(uint32_t)((key >> 2) & 0x3fffffffu)) & 0x3fffffffu);
      nd.t = (int32_t)(key & 3u);
      if (row) { nd.i = (uint64_t)(k * bm + idx / n); nd.j = (uint64_t)(1 + idx % n); }
      else { nd.j = (uint64_t)(k * bn + idx / m); nd.i = (uint64_t)(1 + idx % m); }
    };
    int32_t vr, vc;
    msa_node br, bc;
    decode(hk[2 * k], true, vr, br);
    decode(hk[2 * k + 1], false, vc, bc);
    part.push_back(vr > vc ? br : bc);  // partial.cpp:131-135: ties go to the column
  }
  part.push_back(msa_node{(uint64_t)m, (uint64_t)n, 1, 0});
  // partial.cpp:141-143: std::sort with the reference's comparator.  Past 16 elements
  // std::sort (introsort) is not stable, so points that tie on (i, j) -- the (0,0,0) of a
  // band with no cell above INT_MIN when p > m or p > n -- land where libstdc++'s introsort
  // puts them; the same header algorithm on the same sequence of comparisons reproduces the
  // reference's order (tests/golden/partial_ties.json, made by the reference's build).
  std::sort(part.begin(), part.end(), [](const msa_node& a, const msa_node& b) {
    return (a.i < b.i) || (a.i == b.i && a.j < b.j);
  });
  return part;
}

}  // namespace msa_host

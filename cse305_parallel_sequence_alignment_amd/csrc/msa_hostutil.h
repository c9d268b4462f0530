// msa_hostutil.h -- the pure host-side steps of the host-pointer entries (msa_capi.hip, msa_refapi.inc,
// msa_alignapi.inc): symbol codes, CIGAR strings, the border gap, plan descriptions.  Standard C++ only -- no HIP --
// so that tests/cpp/hostutil_driver.cpp runs every one of them on the CPU under sanitizers.  (msa_refwalk.h: the
// reference API's own rules, in the same way.)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "msa.h"

namespace msa_host {

// Symbols -> codes.  A new symbol takes the next code, in first-seen order, while fewer than `limit` have one
// (MSA_ERR_ALPHABET after that); `preset`'s symbols hold codes 0, 1, ... from the start ("ACGT": every DNA call
// shares one code map).  After fix() no symbol gets a new code: a fixed map over the symbols add()ed so far.
class SymbolMap {
 public:
  explicit SymbolMap(int limit, const char* preset = "") : limit_(limit) {
    std::fill(code_, code_ + 256, -1);
    for (; *preset; ++preset) add(*preset);
  }
  // the next code for c; false if c has one already or the limit is reached
  bool add(char c) {
    int& code = code_[(unsigned char)c];
    if (code >= 0 || next_ >= limit_) return false;
    code = next_++;
    return true;
  }
  void fix() { limit_ = next_; }
  int size() const { return next_; }
  int encode(const char* s, size_t len, uint8_t* out) {
    for (size_t k = 0; k < len; ++k) {
      int code = code_[(unsigned char)s[k]];
      if (code < 0) {
        if (!add(s[k])) return MSA_ERR_ALPHABET;
        code = next_ - 1;
      }
      out[k] = (uint8_t)code;
    }
    return MSA_OK;
  }

 private:
  int code_[256];
  int limit_, next_ = 0;
};

// The run-length string, start -> end, of ops given end -> start ("MMDM" from the end is 1M1D2M).
inline std::string cigar_of(const char* ops, size_t n_ops) {
  std::string c;
  for (size_t k = n_ops; k > 0;) {
    const char op = ops[k - 1];
    size_t run = 0;
    while (k > 0 && ops[k - 1] == op) { run++; k--; }
    c += std::to_string(run);
    c.push_back(op);
  }
  return c;
}

// A device walk stops on the matrix border at (i, j); what is left of the alignment is one gap along that border.
// global: i x 'I', else j x 'D'.  fit: i x 'I' only -- the reference's symbols before column j are free, the
// aligned substring starts there.  none (a local alignment): nothing.  Returns j.
enum Border { BORDER_NONE, BORDER_GLOBAL, BORDER_FIT };
inline int64_t complete_border(std::string& ops, int64_t i, int64_t j, Border rule) {
  if (rule != BORDER_NONE && i > 0) ops.append((size_t)i, 'I');
  else if (rule == BORDER_GLOBAL && j > 0) ops.append((size_t)j, 'D');
  return j;
}

// A banded extension's clip rule (msa.h at msa_extend_align_banded): rows past n + band and columns past m + band hold
// no cell with |i - j| <= band, so the problem is the pair of prefixes (m', n') = (min(m, n + band), min(n, m + band)),
// which always has |m' - n'| <= band.  false for m, n < 1 or band < 0
inline bool extend_band_clip(int64_t m, int64_t n, int64_t band, int64_t& m_eff, int64_t& n_eff) {
  if (m < 1 || n < 1 || band < 0) return false;
  // (n + band may pass INT64_MAX for a huge band: compare the differences instead)
  m_eff = (m - n > band) ? n + band : m;
  n_eff = (n - m > band) ? m + band : n;
  return true;
}

// The description of a plan for one pair spread over many workgroups, with the arrays it points to (so: neither
// copied nor moved).  No band, codes at offset 0; the caller sets the scores.
struct SinglePairDesc {
  msa_plan_desc d;
  SinglePairDesc(int alg, int cells, int64_t m, int64_t n) : m_(m), n_(n) {
    std::memset(&d, 0, sizeof(d));
    d.alg = alg;
    d.cells = cells;
    d.band = -1;
    d.single = 1;
    d.n_pairs = 1;
    d.m = &m_;
    d.n = &n_;
    d.a_off = d.b_off = &zero_;
  }
  SinglePairDesc(const SinglePairDesc&) = delete;
  SinglePairDesc& operator=(const SinglePairDesc&) = delete;

 private:
  int64_t m_, n_, zero_ = 0;
};

// Byte offsets (k + 1 of them) of a batch walk's ops: pair p gets m[p] + n[p] + 2 bytes rounded up to 16, back to
// back (Plan.ops_layout in plan.py is the same rule).
inline std::vector<int64_t> ops_offsets(const int64_t* m, const int64_t* n, int64_t k) {
  std::vector<int64_t> off((size_t)k + 1, 0);
  for (int64_t p = 0; p < k; ++p) off[(size_t)p + 1] = off[(size_t)p] + ((m[p] + n[p] + 2 + 15) & ~int64_t(15));
  return off;
}

}  // namespace msa_host

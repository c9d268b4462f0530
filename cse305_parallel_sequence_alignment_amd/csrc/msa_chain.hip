// msa_chain.hip -- seed chaining (msa_chain_run; the contract is include/msa.h's at msa_chain_seeds): for every anchor
// of a problem the best score of a colinear chain ending there, f, and the predecessor that gives it, pred.
//
//   cand(j, i) = f(j) + match min(da, db, len_i) - gc(|da - db|),  da = ae_i - ae_j, db = be_i - be_j, j < i admissible
//   f(i)       = max(match len_i, max cand(j, i));  pred(i) = the LARGEST j with cand(j, i) == f(i) > match len_i, else -1
//
// The schedule is msa_xdrop.hip's: one WAVE per problem, CH_WPB problems per workgroup, nothing shared between waves:
// no barrier at all, no hand-off word, no spin wait.  Every loop is bounded by N and the lookback.
//
// A wave takes its anchors 64 at a time, lane l anchor i0 + l (one coalesced load of a, b and len; the next 64 are
// loaded while these are worked on), and walks them one by one: anchor i's ae, be and len reach every lane by
// v_readlane.  The window i-1, i-2, ..., max(0, i - lookback) is taken in chunks of 64, nearest first, lane l of chunk c
// at j = i - 1 - 64 c - l.  be ascends with the index, so db only grows along the window: after a chunk in which some
// lane saw db > max_dist no further chunk holds an admissible j, and the walk of the window stops there.
//
// The tie rule.  A lane meets its j in descending order and keeps a candidate only if it is strictly greater, so it
// holds its largest j of its best value.  After the window: one wave-wide maximum of the values, then the largest j
// among the lanes that hold it -- in a one-chunk window (every window of a lookback <= 64) lane order is descending j,
// so that is the first such lane of a ballot; else a second wave-wide maximum, of j.
//
// The ring.  ae, be and f of the window live in a per-wave LDS ring of R = ch_ring_ints(lookback) =
// 64 ceil(lookback / 64) + 64 entries each, >= lookback + 64: the 64 anchors of a block write their ae and be at once
// (slots (i0 mod R) + l; R is a multiple of 64, so a block never wraps inside itself) and overwrite only anchors below
// i0 + 63 - R < i0 - lookback, which no window of this block reaches.  f(i) is one lane's store per anchor, ordered
// before the next anchor's reads by xd_wave_sync; f never goes through global memory and back.  At the cap, lookback
// 1,024: 4 waves x 3 arrays x 1,088 x 4 B = 52,224 B of dynamic LDS, inside a workgroup's 64 KiB.
// f(i) and pred(i) stay in lane (i mod 64)'s registers until the block is done and leave as two coalesced stores.
//
// Values.  Coordinates are within [0, 2^26], match 2^26 < 2^30 and gc(min(band, 2^26)) < 2^30 (the entries check the
// parameters, the kernel each problem's anchors): f(i) <= match ae_i by induction, so every sum fits an int32.
//
// A problem whose anchors break a rule (a negative coordinate, len < 1, an end above 2^26, (be, ae) descending, or
// offsets that are negative, descending or more than 2^26 apart) gets status MSA_ERR_ARG and NOTHING else is written for
// it: the checks are a pass of their own over the anchors before the first f.  N = 0 is status 0 and writes nothing.
//
// Expected latency per anchor (an expectation written before the first run, from the X-drop family's figures, DESIGN
// section 10 item 12: ~0.3 us per dependent step of one chunk, ~0.19 us per wave-wide maximum): the chain f(i-1) -> LDS
// -> cand -> wave maximum -> readfirstlane -> f(i) -> LDS is one such step with one maximum whatever the lookback, so
// ~0.5 us per anchor at lookback 64.  Beyond one chunk the second maximum adds ~0.19 us, and each further chunk three
// LDS reads and ~15 vector instructions that do not wait on f(i-1) -- without the X-drop chunks' global loads, so ~0.1
// rather than 0.35 us each: ~0.9 us at lookback 256, ~2.2 us at 1,024.  What was measured is in DESIGN section 8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msa_xdrop.hip"

namespace msa {

constexpr int CH_WPB = 4;               // problems (waves) per workgroup
constexpr int CH_LOOKBACK_MAX = 1024;   // MSA_CHAIN_LOOKBACK_MAX
constexpr int CH_LIMIT = 1 << 26;       // coordinates, and anchors per problem

__host__ __device__ constexpr int ch_ring_ints(int lookback) { return (lookback + 63) / 64 * 64 + 64; }
__host__ __device__ constexpr size_t ch_lds_bytes(int lookback) {
  return (size_t)CH_WPB * 3 * ch_ring_ints(lookback) * 4;
}
static_assert(ch_ring_ints(CH_LOOKBACK_MAX) == 1088 && ch_lds_bytes(CH_LOOKBACK_MAX) == 52224, "the header's figures");
static_assert(ch_lds_bytes(CH_LOOKBACK_MAX) <= 65536, "a workgroup's LDS");

// Wave v of block b chains problem p = b * CH_WPB + v: anchors off[p] .. off[p + 1] of a, b, len.  h = gap_open -
// gap_extend, g = gap_extend; band and max_dist are clamped to 2^26 by the launcher.  f, pred: per anchor, pred an index
// within the problem; status: per problem.
__global__ __launch_bounds__(64 * CH_WPB) void chain_kernel(
    const long long* __restrict__ a, const long long* __restrict__ b, const long long* __restrict__ len, int n_problems,
    const long long* __restrict__ off, int match, int h, int g, int band, int max_dist, int lookback,
    int* __restrict__ f, int* __restrict__ pred, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) int ch_lds[];
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int p = (int)blockIdx.x * CH_WPB + wave;
  if (p >= n_problems) return;
  const int R = ch_ring_ints(lookback);
  int* AE = ch_lds + wave * 3 * R;
  int* BE = AE + R;
  int* F = BE + R;

  const long long o0 = off[p], o1 = off[p + 1];
  if (o0 < 0 || o1 < o0 || o1 - o0 > CH_LIMIT) {
    if (lane == 0) status[p] = MSA_ERR_ARG;
    return;
  }
  const int N = (int)(o1 - o0);
  const long long* pa = a + o0;
  const long long* pb = b + o0;
  const long long* pl = len + o0;

  // the problem's own checks, before anything is written for it
  bool bad = false;
  for (int t0 = 0; t0 < N; t0 += 64) {
    const int t = t0 + lane;
    if (t < N) {
      const long long x = pa[t], y = pb[t], l = pl[t];
      bool ok = x >= 0 && y >= 0 && l >= 1 && x <= CH_LIMIT && y <= CH_LIMIT && l <= CH_LIMIT && x + l <= CH_LIMIT &&
                y + l <= CH_LIMIT;
      if (ok && t > 0) {
        const long long x0 = pa[t - 1], y0 = pb[t - 1], l0 = pl[t - 1];
        // (a predecessor out of range is its own lane's finding)
        if (x0 >= 0 && y0 >= 0 && l0 >= 1 && x0 <= CH_LIMIT && y0 <= CH_LIMIT && l0 <= CH_LIMIT)
          ok = y + l > y0 + l0 || (y + l == y0 + l0 && x + l >= x0 + l0);
      }
      bad = bad || !ok;
    }
  }
  if (__any(bad)) {
    if (lane == 0) status[p] = MSA_ERR_ARG;
    return;
  }
  if (lane == 0) status[p] = 0;
  if (N == 0) return;

  int* pf = f + o0;
  int* pp = pred + o0;
  // lane l's anchor of the next block of 64, loaded one block ahead
  int n_ae = 0, n_be = 0, n_len = 0;
  if (lane < N) {
    const int l = (int)pl[lane];
    n_ae = (int)pa[lane] + l;
    n_be = (int)pb[lane] + l;
    n_len = l;
  }
  int s0 = 0;  // i0 mod R
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int my_ae = n_ae, my_be = n_be, my_len = n_len;
    {
      const int t = i0 + 64 + lane;
      if (t < N) {
        const int l = (int)pl[t];
        n_ae = (int)pa[t] + l;
        n_be = (int)pb[t] + l;
        n_len = l;
      }
    }
    AE[s0 + lane] = my_ae;
    BE[s0 + lane] = my_be;
    xd_wave_sync();
    const int cnt = min(64, N - i0);
    int out_f = 0, out_p = -1;
    for (int u = 0; u < cnt; ++u) {
      const int i = i0 + u, si = s0 + u;
      const int ae_i = __builtin_amdgcn_readlane(my_ae, u), be_i = __builtin_amdgcn_readlane(my_be, u);
      const int len_i = __builtin_amdgcn_readlane(my_len, u);
      const int base = match * len_i;
      const int lo = max(0, i - lookback);
      int bc = INT32_MIN, bj = -1;  // this lane's best candidate and its largest j
      for (int j0 = i - 1; j0 >= lo; j0 -= 64) {
        const int j = j0 - lane;
        bool far = false;
        if (j >= lo) {
          int s = si - (i - j);  // i - j <= lookback < R
          s = s < 0 ? s + R : s;
          const int da = ae_i - AE[s], db = be_i - BE[s], fj = F[s];
          const int skew = da > db ? da - db : db - da;
          far = db > max_dist;
          if (da > 0 && db > 0 && da <= max_dist && !far && skew <= band) {
            const int c = fj + match * min(min(da, db), len_i) - (skew ? h + g * skew : 0);
            if (c > bc) bc = c, bj = j;
          }
        }
        if (__any(far)) break;
      }
      int fi = base, pi = -1;
      const int m = xd_wave_max(bc);
      if (m > base) {
        fi = m;
        if (i - lo <= 64) {  // one chunk: lane order is descending j
          const unsigned long long hit = __ballot(bc == m);
          pi = i - 1 - (int)__builtin_ctzll(hit);
        } else {
          pi = xd_wave_max(bc == m ? bj : -1);
        }
      }
      if (lane == 0) F[si] = fi;
      if (lane == u) out_f = fi, out_p = pi;
      xd_wave_sync();
    }
    if (lane < cnt) {
      pf[i0 + lane] = out_f;
      pp[i0 + lane] = out_p;
    }
    s0 += 64;
    if (s0 == R) s0 = 0;
  }
}

}  // namespace msa

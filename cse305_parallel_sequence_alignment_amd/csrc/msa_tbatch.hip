// msa_tbatch.hip -- many short traceback walks in one launch (msa_plan_traceback_batch).
//
// traceback_kernel (msa_traceback.hip) spends a six-wave workgroup and ~86 KiB of LDS on one walk: the right
// trade for one 97k-row pair, the wrong one for a batch of read-sized pairs, which it walks one launch and one
// CU at a time.  Here one WAVE walks one pair and a workgroup holds TBB_WPB independent walks; a launch walks
// every pair of the plan.
//
// The bytes, the skewed stripe layout, the transitions and their tie order are msa_traceback.hip's (TB_SW and
// TB_NW, one row per lane, stripe starts from the stripe meta; TB_FIT: TB_NW from each pair's end cell).  What differs:
//  * a wave stages its own groups.  It owns one LDS slot of TBB_GB consecutive 1 KiB blocks of one stripe,
//    fills it by LDS-DMA (glds16x16, or glds16 with the last block repeated for a stripe of fewer blocks),
//    waits with its own s_waitcnt vmcnt(0) and walks the slot with the run / window loop of the single
//    walker.  A new group is staged when the walk enters a stripe (the group ending 16 steps right of the
//    entry step: group_b0's rule) or leaves its group on the left.  No prefetch: the load latency of one
//    group per stripe is on the walk, and the other walks of the CU hide it.
//  * a wave writes its own ops, with per-lane byte stores: a run of q stores 'M' from lanes < q; a window
//    stores step k's op from lane k < 7 at the number of op-producing steps before it.  Every store is
//    guarded by its index < capacity; the count runs on, so a short buffer gives MSA_ERR_CAPACITY and its
//    true length.  No ring, no decoder.
//  * the pair's stripe start columns are staged in the wave's LDS once (TBB_CSN of them; a pair with more
//    stripes reads the rest from memory), so a stripe change costs an LDS read.
// After the early return of the waves without a pair nothing in the kernel is shared between waves: no
// barrier, no hand-off word, no spin wait.  A walk waits for its own loads only.
//
// Every loop ends, whatever bytes dDir holds (the GPU is shared; a walk over garbage must not keep a wave):
// a pass of the inner loop either moves the walk (lane 0 of a window holds the walk's own cell: states E and
// F always step, state H steps, stops or enters E / F) or leaves the loop, and i + j only decreases; the
// outer loop (one pass per stripe or group change) counts its passes and ends the walk with MSA_ERR_TIMEOUT
// beyond m + n + 2 stripes + 8.  A step outside the stripe's blocks (never reached over a fill's bytes) ends
// the walk with MSA_ERR_NOMATCH before anything is loaded from there.
#pragma once
#include "msa_traceback.hip"

namespace msa {

constexpr int TBB_WPB = 4;       // walks (waves) per workgroup
constexpr int TBB_GB = 16;       // blocks per group: 256 steps x 64 rows, 16 KiB
constexpr int TBB_GUARD = 2304;  // in front of the first slot (traceback_kernel's: window lanes outside a group)
constexpr int TBB_CSN = 512;     // stripe starts staged per walk (32k rows)
// LDS per walk: 16 KiB + 2 KiB + 576 B = 18,944 B (<= 20 KiB: 8 walks per CU)

// the first block of the group of a stripe of pmax blocks that ends a little right of step t (group_b0)
__device__ __forceinline__ int tbb_group_b0(int t, int pmax) {
  int b0 = ((t + 16) >> 4) - (TBB_GB - 1);
  b0 = b0 < pmax - TBB_GB ? b0 : pmax - TBB_GB;
  return b0 > 0 ? b0 : 0;
}

// Wave w of block b walks pair b * TBB_WPB + w.  ops_off: n_pairs + 1 non-decreasing byte offsets into ops_base
// (pair p's capacity = ops_off[p + 1] - ops_off[p]).  info[8 p ..]: {n_ops, i + 1, j + 1, status, stripes
// entered, groups staged, s_memtime ticks, 0}, words 0-3 as traceback_kernel writes them.
template <int KIND>
__global__ __launch_bounds__(64 * TBB_WPB) void traceback_batch_kernel(
    const uint8_t* __restrict__ dir, const msa_pair_desc* __restrict__ pairs, const msa_stripe_meta* __restrict__ meta,
    const PairResult* __restrict__ res, int n_pairs, uint8_t* __restrict__ ops_base,
    const long long* __restrict__ ops_off, long long* __restrict__ info) {
  static_assert(KIND == TB_SW || KIND == TB_NW || KIND == TB_FIT, "one row per lane, SW-affine bytes");
  // a global walk: from (m, n) -- TB_FIT: from the pair's end cell (m, end_j) -- to the matrix border
  constexpr bool REF = KIND == TB_NW || KIND == TB_FIT;
  constexpr int GB = TBB_GB, GT = 16 * GB, GBYTES = 1024 * GB;
  __shared__ __attribute__((aligned(16))) uint8_t stage_raw[TBB_GUARD + TBB_WPB * GBYTES];
  __shared__ int csl[TBB_WPB][TBB_CSN];
  typedef __attribute__((address_space(3))) uint8_t lds_u8;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int pair = (int)blockIdx.x * TBB_WPB + wave;
  if (pair >= n_pairs) return;

  const msa_pair_desc pd = pairs[pair];
  const uint8_t* base = dir + pd.out_off + lane * 16;
  const int pmax = pd.pmax;
  const int S = (pd.m + 63) / 64;
  // (a flat pointer to LDS holds the LDS address in its low 32 bits)
  const unsigned grp_lds = (unsigned)(uintptr_t)&stage_raw[TBB_GUARD] + (unsigned)GBYTES * (unsigned)wave;
  const long long off0 = ops_off[pair], cap64 = ops_off[pair + 1] - off0;
  uint8_t* ops = ops_base + off0;
  // (a walk has fewer than 2^27 ops: plans hold m, n < 2^26)
  const int cap = cap64 < 0 ? 0 : (cap64 > (1ll << 30) ? (1 << 30) : (int)cap64);
  for (int k = lane; k < S && k < TBB_CSN; k += 64) csl[wave][k] = meta[pd.stripe0 + k].cs;
  auto cs_of = [&](int k) {  // wave-uniform (readfirstlane: an LDS value is otherwise "divergent")
    return k < TBB_CSN ? __builtin_amdgcn_readfirstlane(csl[wave][k]) : meta[pd.stripe0 + k].cs;
  };

  const long long t_begin = (long long)__builtin_amdgcn_s_memtime();
  int i, j, status = 0, n_switch = 0, n_grp = 0, o = 0;
  bool walk = true;
  if constexpr (KIND == TB_NW) {
    i = pd.m;
    j = pd.n;
  } else {
    const PairResult r0 = res[pair];
    i = (int)r0.end_i;
    j = (int)r0.end_j;
    // (a fit alignment exists whatever its score.  An overlap plan's pairs walk as TB_FIT too: its empty overlap --
    // score 0, the only score <= 0 it reports -- has the end cell (m, 0), so `j > 0` below ends that walk before its
    // first step with n_ops 0; no score test is needed, and none is passed in)
    walk = KIND == TB_FIT || r0.score > 0;
    // (an end cell outside the matrix: the plan has not run)
    if (r0.end_i < 0 || r0.end_i > pd.m || r0.end_j < 0 || r0.end_j > pd.n) {
      status = MSA_ERR_ARG;
      walk = false;
    }
  }
  // windows: lane (a, b) = (lane >> 3, lane & 7) holds cell (i - a, j - b) (traceback_kernel)
  const int wa = lane >> 3, wb = lane & 7;
  const int wc = wa + wb, wa16 = 16 * wa;
  constexpr unsigned FROZEN = (10u << 10) | (20u << 20) | (1u << 31);
  if (walk) {
    bool stopped = false;
    int st = 0;  // 0 in H, 1 in E (horizontal gap), 2 in F (vertical gap)
    int s_cur = -1, cs = 0, g_s = -1, g_b0 = 0;
    const int pass_max = pd.m + pd.n + 2 * S + 8;
    int pass = 0;
    // outer pass: the walk entered a stripe, or left its group on the left
    while (i > 0 && j > 0 && !stopped && status == 0) {
      if (++pass > pass_max) {
        status = MSA_ERR_TIMEOUT;
        break;
      }
      const int s = (i - 1) >> 6;
      int r = (i - 1) & 63;  // row in the stripe
      if (s != s_cur) {
        cs = cs_of(s);
        s_cur = s;
        ++n_switch;
      }
      const int t = j - cs + r;
      if (t < 0 || t >= 16 * pmax) {  // outside the stripe's blocks
        status = MSA_ERR_NOMATCH;
        break;
      }
      if (g_s != s || t < 16 * g_b0 || t >= 16 * g_b0 + GT) {
        // stage the group of stripe s covering step t (always 16 loads), wait for it
        g_s = s;
        g_b0 = tbb_group_b0(t, pmax);
        if (pmax >= GB) {
          glds16x16(base + ((long long)s * pmax + g_b0) * 1024, grp_lds);
        } else {
#pragma unroll
          for (int q = 0; q < GB; ++q) {
            const int qb = q < pmax ? q : pmax - 1;  // (a short stripe loads its last block again)
            glds16(base + ((long long)s * pmax + qb) * 1024, grp_lds + 1024u * q);
          }
        }
        ++n_grp;
        vm_wait_all();
      }
      int tg = t - 16 * g_b0;
      int sh = 10 * st;
      for (;;) {
        if (sh == 0) {
          // diagonal run: lane q reads cell (i - q, j - q) (inside the group and the matrix for q <= qmax);
          // the run is the number of leading lanes that continue diagonally in state H
          int qmax = r < (tg >> 1) ? r : (tg >> 1);
          qmax = qmax < i - 1 ? qmax : i - 1;
          qmax = qmax < j - 1 ? qmax : j - 1;
          const bool valid = lane <= qmax;
          const int tt = tg - 2 * lane, rr = r - lane;
          const unsigned go = (unsigned)(((tt >> 4) << 10) + (rr << 4) + (tt & 15));
          const unsigned dv = *(const lds_u8*)(uintptr_t)(grp_lds + (valid ? go : 0u));
          const unsigned long long bal = __ballot(valid && tb_diag_stay<KIND>(dv));
          const int q = ~bal == 0ull ? 64 : (int)__builtin_ctzll(~bal);
          if (q > 0) {
            if (lane < q && o + lane < cap) ops[o + lane] = 'M';
            o += q;
            tg -= 2 * q;
            r -= q;
            i -= q;
            j -= q;
            if (r < 0 || tg < 0 || i <= 0 || j <= 0) break;
          }
        }
        // a window of seven steps
        int wt;
        {
          const int d = (tg & 15) - wc;
          const unsigned ga = grp_lds + (unsigned)(((tg >> 4) << 10) + (r << 4)) + (unsigned)(d + 1008 * (d >> 4) - wa16);
          const bool live = wa <= min(r, i - 1) && wb <= j - 1 && wc <= tg;
          const unsigned dv = *(const lds_u8*)(uintptr_t)ga;
          const unsigned w = tb_word<KIND>(dv);  // (evaluated for every lane: a select, no branch)
          wt = (int)(live ? w : FROZEN);
        }
        int idx = 0;
        unsigned wcode = 0;
#pragma unroll
        for (int kk = 0; kk < 7; ++kk) {
          const unsigned long long w64 = (7ull << 32) | (unsigned)__builtin_amdgcn_readlane(wt, idx);
          const unsigned f = (unsigned)(w64 >> (sh & 63));
          const unsigned dl = (f >> 6) & 15u;
          sh = (int)f;
          idx += (int)dl;
          wcode = (wcode << 4) + dl;
        }
        sh &= 31;
        // step k's lane step is nibble 6 - k of the (uniform) code word: 9 'M', 1 'D', 8 'I', 0 no op
        unsigned nz = wcode | (wcode >> 1);
        nz = (nz | (nz >> 2)) & 0x1111111u;  // bit 4q: nibble q is not 0
        if (lane < 7) {
          const int nb = 4 * (6 - lane);
          const unsigned dl = (wcode >> nb) & 15u;
          const int at = o + __popc(nz >> (nb + 4));  // op-producing steps before this one
          if (dl != 0u && at < cap) ops[at] = dl == 9u ? 'M' : (dl == 1u ? 'D' : 'I');
        }
        o += __popc(nz);
        const int da = idx >> 3, db = idx & 7;
        tg -= da + db;
        r -= da;
        i -= da;
        j -= db;
        // stop; or the walk left the group (top row or left edge) or reached the border
        if (sh == 30 || r < 0 || tg < 0 || i <= 0 || j <= 0) break;
      }
      st = (sh == 30) ? 3 : sh / 10;
      if constexpr (REF) {
        // a cell without a predecessor (cannot happen for a complete fill)
        if (st == 3) {
          status = MSA_ERR_NOMATCH;
          stopped = true;
        }
      } else if (st == 3) {  // local start (H came from 0): the walk ends at this cell
        st = 0;
        stopped = true;
      }
    }
  }
  const long long ticks = (long long)__builtin_amdgcn_s_memtime() - t_begin;
  if (lane == 0) {
    if (o > cap && status == 0) status = MSA_ERR_CAPACITY;
    long long* out = info + 8ll * pair;
    out[0] = o;
    out[1] = i + 1;
    out[2] = j + 1;
    out[3] = status;
    out[4] = n_switch;
    out[5] = n_grp;
    out[6] = ticks;
    out[7] = 0;
  }
}

}  // namespace msa

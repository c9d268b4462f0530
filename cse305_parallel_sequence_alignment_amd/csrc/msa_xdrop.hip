// msa_xdrop.hip -- banded extension alignment with X-drop termination (msa_xdrop_extend_run, msa_xdrop_flank_run,
// msa_xdrop_extend_walk; the contract is include/msa.h's at msa_extend_align_xdrop).
//
// The stripe kernel lays its phases, barriers and hand-offs out from m, n and the band before the launch, so it
// computes every cell of its schedule.  A data-dependent stop needs a schedule without cross-wave dependencies:
// here one WAVE fills one pair, XD_WPB pairs per workgroup (msa_tbatch.hip's shape), anti-diagonal by anti-diagonal,
// and decides after each whether to go on.  After the table is staged (one barrier) nothing is shared between waves:
// no barrier, no hand-off word, no spin wait.  Every loop is bounded by m + n.
//
// Cells.  d = i + j; in band form cell (i, j) has k = j - i + w in [0, 2w], and on one anti-diagonal k = d - 2i + w
// has the parity of d + w.  Its neighbours: left (i, j-1) is (d-1, k-1), up (i-1, j) is (d-1, k+1), diagonal
// (i-1, j-1) is (d-2, k).  So ONE array of 2w + 1 slots per state holds both earlier anti-diagonals: the slots of d's
// parity hold d - 2 and are overwritten by d (each lane reads its own slot before it writes it), the others hold
// d - 1 and are only read.  Slot k sits at index k + 1; indices 0 and 2w + 2 are never written and stay -inf: the
// out-of-band neighbours.  The matrix borders (0, d) and (d, 0) are written into H's slots w + d and w - d as the
// sweep passes anti-diagonal d <= w (no interior cell uses those slots before d + 2); their E and F stay -inf.
// Lanes take the cells of an anti-diagonal (at most w + 1) in chunks of 64, rows ascending.
//
// LDS: 1 KiB of scores (int8, stride 32: one instantiation for 3-bit and 5-bit codes) + per wave 3 int32 arrays of
// 2w + 4.  XD_BAND_MAX = 640: 1,024 + 4 x 3 x 1,284 x 4 = 62,656 B, inside a workgroup's 64 KiB, and two workgroups
// (eight pairs) fit a CU's 160 KiB at the cap.
//
// Values.  -inf is XD_NEG = -2^30; the value-range inequality of msa_plan_create_scored (checked per pair, status
// MSA_ERR_UNSUPPORTED) keeps every finite value above -2^28, and E and F are set back to XD_NEG whenever they fall
// below -2^29, so a -inf never drifts.  The diagonal term is always finite (a cell's diagonal neighbour is in the
// band or on a border inside it), hence so is H.
//
// The direction bytes (format: msa_plan_traceback_nw's) go to a compact band form of their own: cell (i, j) of pair p
// at dir_off[p] + i (2w + 1) + k, rows 0 .. m.  The walk kernel (one wave per pair again) reads them back from the
// end cell: lane q looks at (i - q, j - q), so a diagonal run of up to 64 'M' is one step; gap steps go one by one.
// A walk over a fill's bytes only meets cells with a smaller i + j than the end cell's, all of them computed; over
// anything else it still ends: every pass moves the walk or changes H to a gap state that moves in the next, a count
// of the passes ends it with MSA_ERR_TIMEOUT beyond 2 (i + j) + 4, and a step out of the band is MSA_ERR_NOMATCH
// before anything is read there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msa {

constexpr int XD_WPB = 4;          // pairs (waves) per workgroup
constexpr int XD_BAND_MAX = 640;   // MSA_XDROP_BAND_MAX
constexpr int XD_NEG = -(1 << 30);
constexpr int XD_NONE = INT32_MIN;  // MSA_SCORE_NONE

__host__ __device__ constexpr int xd_row_ints(int w) { return 2 * w + 4; }
__host__ __device__ constexpr size_t xd_lds_bytes(int w) { return 1024 + (size_t)XD_WPB * 3 * xd_row_ints(w) * 4; }
static_assert(xd_lds_bytes(XD_BAND_MAX) <= 65536, "a workgroup's LDS");

__device__ __forceinline__ int xd_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return __builtin_amdgcn_readfirstlane(v);
}

// what the lanes of one wave wrote to LDS is what they read next (LDS serves a wave's accesses in order; this keeps
// the compiler from moving them across)
__device__ __forceinline__ void xd_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Wave v of block b fills pair b * XD_WPB + v: A[pa .. + m) against B[pb .. + n), |m - n| <= w.  step (nullptr: every
// pair +1): the pair's reading direction s, +1 or -1 (anything else: status MSA_ERR_ARG) -- row i's code is
// A[pa + s (i - 1)], column j's is B[pb + s (j - 1)], so with s = -1 the pair is the sequences that END at pa and pb,
// read backwards in place (a seed's left flank); s is wave-uniform and only the two code loads know of it: the cells,
// the tracker, the bytes and the result are in the pair's own (flank) coordinates, and the table is never transposed.
// STEP = (step != nullptr), the launcher's choice: a launch without steps runs the instantiation that has none in it.
// sub32: 1,024 int8 scores at stride 32 (row: A's code), or nullptr: match / mismatch.  g = gap_extend, op = gap_open.
// xdrop < 0: never stop.  dir may be nullptr (no bytes).  res[8 p ..] = {score, end_i, end_j, D, H(m, n) or XD_NONE,
// status, cells computed, 0}.
template <bool STEP>
__global__ __launch_bounds__(64 * XD_WPB) void xdrop_fill_kernel(
    const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, int n_pairs, const long long* __restrict__ pm,
    const long long* __restrict__ pn, const long long* __restrict__ pa, const long long* __restrict__ pb,
    const int8_t* __restrict__ step, const int8_t* __restrict__ sub32, int match, int mismatch, int g, int op, int w, int xdrop,
    uint8_t* __restrict__ dir, const long long* __restrict__ dir_off, long long* __restrict__ res) {
  extern __shared__ __attribute__((aligned(16))) int xd_lds[];
  int8_t* stab = (int8_t*)xd_lds;
  for (int t = (int)threadIdx.x; t < 1024; t += 64 * XD_WPB)
    stab[t] = sub32 ? sub32[t] : (int8_t)((t >> 5) == (t & 31) ? match : mismatch);
  __syncthreads();
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int pair = (int)blockIdx.x * XD_WPB + wave;
  if (pair >= n_pairs) return;

  const int W2 = xd_row_ints(w);
  int* Hs = xd_lds + 256 + wave * 3 * W2;
  int* Es = Hs + W2;
  int* Fs = Es + W2;
  const long long m64 = pm[pair], n64 = pn[pair];
  int smax = 0;
  for (int t = lane; t < 1024; t += 64) {
    const int v = stab[t];
    smax = max(smax, v < 0 ? -v : v);
  }
  smax = xd_wave_max(smax);
  const int s = STEP ? __builtin_amdgcn_readfirstlane((int)step[pair]) : 1;
  int status = 0;
  if (m64 < 1 || n64 < 1 || m64 > (1 << 26) || n64 > (1 << 26) || m64 - n64 > w || n64 - m64 > w || (s != 1 && s != -1))
    status = MSA_ERR_ARG;
  else if (((long long)smax + 2ll * op + 2ll * g) * (m64 + n64 + 256) + ((long long)op - g) >= (1ll << 28))
    status = MSA_ERR_UNSUPPORTED;
  long long* out = res + 8ll * pair;
  if (status != 0) {
    if (lane == 0) {
      out[0] = 0, out[1] = 0, out[2] = 0, out[3] = 0, out[4] = XD_NONE, out[5] = status, out[6] = 0, out[7] = 0;
    }
    return;
  }
  const int m = (int)m64, n = (int)n64, d_end = m + n, h = op - g;
  for (int t = lane; t < 3 * W2; t += 64) Hs[t] = XD_NEG;
  xd_wave_sync();
  if (lane == 0) {
    Hs[w + 1] = 0;
    if (w >= 1) Hs[w + 2] = Hs[w] = -h - g;
  }
  xd_wave_sync();

  // Code t (0-based) of a side is at s t from its first symbol.  A lane's rows ascend and its columns descend with
  // the lane, so with steps each lane keeps its own two bases -- row (i0 + lane)'s code is al[s (i0 - 1)], column
  // (j0 - lane)'s is bl[s (j0 - 1)] -- and the offsets are wave-uniform: scalar arithmetic, one 64-bit add per load
  const uint8_t* a = A + pa[pair];
  const uint8_t* b = B + pb[pair];
  const long long sl = (long long)(s * lane);
  const uint8_t* al = a + sl;
  const uint8_t* bl = b - sl;
  auto code_a = [&](int i0) -> int {  // of row i0 + lane
    if constexpr (STEP) return al[(long long)(s * (i0 - 1))];
    else return a[(i0 + lane) - 1];
  };
  auto code_b = [&](int j0) -> int {  // of column j0 - lane
    if constexpr (STEP) return bl[(long long)(s * (j0 - 1))];
    else return b[(j0 - lane) - 1];
  };
  const int RS = 2 * w + 1;
  uint8_t* dp = dir ? dir + dir_off[pair] : nullptr;
  // rows of anti-diagonal d: 1 <= i <= m, 1 <= d - i <= n, |2 i - d| <= w
  auto lo_of = [&](int d) { return max(max(1, d - n), (d - w + 1) >> 1); };
  auto hi_of = [&](int d) { return min(min(m, d - 1), (d + w) >> 1); };
  int bv = XD_NONE, bi = 0, bj = 0;  // this lane's best cell: ties to the smaller i, then the smaller j
  int best = 0, a_prev = XD_NEG, D = d_end, fin = XD_NONE;
  long long cells = 0;
  // the codes of the next anti-diagonal's first chunk are loaded one anti-diagonal ahead
  int nlo = lo_of(2), nhi = hi_of(2), na = 0, nb = 0;
  if (nlo + lane <= nhi) {
    na = code_a(nlo);
    nb = code_b(2 - nlo);
  }
  for (int d = 2; d <= d_end; ++d) {
    const int ilo = nlo, ihi = nhi, ca0 = na, cb0 = nb;
    if (d < d_end) {
      nlo = lo_of(d + 1);
      nhi = hi_of(d + 1);
      const int i = nlo + lane;
      if (i <= nhi) {
        na = code_a(nlo);
        nb = code_b(d + 1 - nlo);
      }
    }
    int ad = XD_NEG;
    for (int i0 = ilo; i0 <= ihi; i0 += 64) {
      const int i = i0 + lane, j = d - i;
      if (i <= ihi) {
        const int k1 = j - i + w + 1;
        const int ca = i0 == ilo ? ca0 : code_a(i0), cb = i0 == ilo ? cb0 : code_b(d - i0);
        const int hd = Hs[k1], hl = Hs[k1 - 1], hu = Hs[k1 + 1], el = Es[k1 - 1], fu = Fs[k1 + 1];
        int e = max(hl - op, el - g), f = max(hu - op, fu - g);
        e = e < XD_NEG / 2 ? XD_NEG : e;
        f = f < XD_NEG / 2 ? XD_NEG : f;
        const int dg = hd + stab[32 * ca + cb];
        const int hv = max(dg, max(e, f));
        Hs[k1] = hv;
        Es[k1] = e;
        Fs[k1] = f;
        if (dp) {
          const int byte = (hv == dg ? 1 : (hv == e ? 2 : 3)) | ((e == hl - op && hl > XD_NEG / 2) ? 4 : 0) |
                           ((f == hu - op && hu > XD_NEG / 2) ? 8 : 0);
          dp[(long long)i * RS + (k1 - 1)] = (uint8_t)byte;
        }
        ad = max(ad, hv);
        if (hv > bv || (hv == bv && (i < bi || (i == bi && j < bj)))) bv = hv, bi = i, bj = j;
        if (i == m && j == n) fin = hv;
      }
    }
    if (lane == 0 && d <= w) Hs[w + d + 1] = Hs[w - d + 1] = -h - g * d;
    xd_wave_sync();
    if (ihi >= ilo) cells += ihi - ilo + 1;
    if (xdrop >= 0) {
      ad = xd_wave_max(ad);
      best = max(best, ad);
      const int recent = max(a_prev, ad);
      a_prev = ad;
      if (best - recent > xdrop) {
        D = d;
        break;
      }
    }
  }
  // the first maximum in row-major order over every lane's cells (all of them have i + j <= D)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int uv = __shfl_xor(bv, o), ui = __shfl_xor(bi, o), uj = __shfl_xor(bj, o);
    if (uv > bv || (uv == bv && (ui < bi || (ui == bi && uj < bj)))) bv = uv, bi = ui, bj = uj;
  }
  fin = xd_wave_max(fin);
  if (lane == 0) {
    const bool empty = bv <= 0;
    out[0] = empty ? 0 : bv;
    out[1] = empty ? 0 : bi;
    out[2] = empty ? 0 : bj;
    out[3] = D;
    out[4] = D == d_end ? fin : XD_NONE;
    out[5] = 0;
    out[6] = cells;
    out[7] = 0;
  }
}

// Wave v of block b walks pair b * XD_WPB + v from its end cell (res, as xdrop_fill_kernel wrote it) over the compact
// band-form bytes.  ops / ops_off / info: traceback_batch_kernel's contract, words 4-7 of info 0.
__global__ __launch_bounds__(64 * XD_WPB) void xdrop_walk_kernel(const uint8_t* __restrict__ dir,
                                                                 const long long* __restrict__ dir_off,
                                                                 const long long* __restrict__ res, int n_pairs, int w,
                                                                 uint8_t* __restrict__ ops_base,
                                                                 const long long* __restrict__ ops_off,
                                                                 long long* __restrict__ info) {
  const int lane = (int)threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int pair = (int)blockIdx.x * XD_WPB + wave;
  if (pair >= n_pairs) return;
  const long long* r = res + 8ll * pair;
  const long long ei = r[1], ej = r[2];
  int status = (int)r[5];
  const long long off0 = ops_off[pair], cap64 = ops_off[pair + 1] - off0;
  const int cap = cap64 < 0 ? 0 : (cap64 > (1ll << 30) ? (1 << 30) : (int)cap64);
  uint8_t* ops = ops_base + off0;
  const uint8_t* dp = dir + dir_off[pair];
  const int RS = 2 * w + 1;
  int i = 0, j = 0, o = 0;
  // (an end cell outside a band-form plane: the fill has not run)
  if (status == 0 && (ei < 0 || ej < 0 || ei > (1 << 26) || ej > (1 << 26) || ei - ej > w || ej - ei > w))
    status = MSA_ERR_ARG;
  if (status == 0) {
    i = (int)ei;
    j = (int)ej;
    int st = 0;  // 0 in H, 1 in E (horizontal gap), 2 in F (vertical gap)
    const int pass_max = 2 * (i + j) + 4;
    int pass = 0;
    while (i > 0 && j > 0) {
      if (++pass > pass_max) {
        status = MSA_ERR_TIMEOUT;
        break;
      }
      const int k = j - i + w;
      if (k < 0 || k > 2 * w) {
        status = MSA_ERR_NOMATCH;
        break;
      }
      if (st == 0) {
        // lane q reads cell (i - q, j - q): the run of leading lanes that go on diagonally
        const bool valid = lane < min(i, j);
        const int v = valid ? (int)dp[(long long)(i - lane) * RS + k] : 0;
        const unsigned long long bal = __ballot(valid && (v & 3) == 1);
        const int q = ~bal == 0ull ? 64 : (int)__builtin_ctzll(~bal);
        if (q > 0) {
          if (lane < q && o + lane < cap) ops[o + lane] = 'M';
          o += q;
          i -= q;
          j -= q;
          continue;
        }
        const int lo = __builtin_amdgcn_readfirstlane(v) & 3;
        if (lo == 0) {  // a cell without a predecessor (cannot happen over a fill's bytes)
          status = MSA_ERR_NOMATCH;
          break;
        }
        st = lo - 1;
      } else {
        const int v = __builtin_amdgcn_readfirstlane((int)dp[(long long)i * RS + k]);
        if (lane == 0 && o < cap) ops[o] = st == 1 ? 'D' : 'I';
        ++o;
        if (st == 1) {
          --j;
          st = (v & 4) ? 0 : 1;
        } else {
          --i;
          st = (v & 8) ? 0 : 2;
        }
      }
    }
  }
  if (lane == 0) {
    if (o > cap && status == 0) status = MSA_ERR_CAPACITY;
    long long* out = info + 8ll * pair;
    out[0] = o;
    out[1] = i + 1;
    out[2] = j + 1;
    out[3] = status;
    out[4] = out[5] = out[6] = out[7] = 0;
  }
}

}  // namespace msa

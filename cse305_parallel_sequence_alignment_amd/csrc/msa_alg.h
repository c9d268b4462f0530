// msa_alg.h -- what each kernel algorithm id (enum msa_alg, msa_types.h) IS: one table, read by the kernels at compile
// time and by the host when it plans, launches and walks.  An id is nothing but its row here; no other file keeps a
// list of ids.  Plain C++17, host and device.
#pragma once
#include "msa_types.h"

// The cell recurrence (step(), msa_kernels.hip).
enum msa_cell {
  CELL_LIN_FLOOR,  // SW linear in G-space, G = H + g (i + j), with the zero floor: one int32 per cell
  CELL_LIN,        // ... without the floor (every substitution score >= 0: it never binds)
  CELL_LIN_PK16,   // ... without the floor, two pairs per lane as packed int16 (score only)
  CELL_SWAFF,      // SW affine: H with the zero floor, E, F
  CELL_GOTOH,      // the reference's Gotoh for start type -1 with g, h >= 0, as H = max(T1, T2, T3), T2, T3
  CELL_REF3,       // the reference's three tables T1, T2, T3, any start type, exact -inf
  CELL_REF_TAG,    // ... for start type -1, values carried tagged as 4 T + (4 - table)
  CELL_PART,       // partial.cpp's three tables with int32 wrap semantics
};

// Row 0 / column 0 of the matrix: the algorithm's gap ramp (for the reference's cells, by start type), or free --
// H = 0 all along, symbols before the alignment cost nothing.
enum msa_border { BORDER_RAMP, BORDER_FREE };

// What a lane tracks beside its cells, and how reduce_pairs_kernel forms a pair's result from the stripe metas.
enum msa_result {
  RES_FINAL = 0,      // the state at (m, n), from the stripe of row m
  RES_BEST = 1,       // the first maximum over all cells under the zero floor (the empty alignment unless positive)
  RES_ROW_M = 2,      // the first maximum of row m, any sign
  RES_ROW_M_COL = 3,  // ... against the last column's, H(i, n), which every stripe keeps (nothing positive: empty)
  RES_BEST_ANY = 4,   // the first maximum over all cells of values that may be negative, with the state at (m, n)
                      // beside it (nothing positive: empty)
};

// Walk kinds (traceback_kernel, traceback_batch_kernel): Smith-Waterman affine from the run's end cell; the
// reference's Gotoh walk over table numbers (REF fill) or over tags (REF1 fill, tag = 4 - table); TB_NW: the global
// walk over SW-affine bytes from (m, n) to the matrix border; TB_FIT: TB_NW's walk -- words, state machine, stop
// rule -- started at the run's end cell from the pair's PairResult: (m, end_j), an overlap's (end_i, n) or (m, 0), an
// extension's anywhere inside or (0, 0) -- the walk loop's `i > 0` / `j > 0` end the empty ones at once.
enum msa_walk { TB_NONE = -1, TB_SW = 0, TB_REF = 1, TB_REF_TAG = 2, TB_NW = 3, TB_FIT = 4 };

#define MSA_ALG_NONE (-1)

struct msa_alg_info {
  int nc;             // values a cell hands to the row below (DPP, rings, granules)
  msa_cell cell;
  msa_border top, left;
  msa_result result;
  bool wide;          // 5-bit codes (a 32-byte profile per row, score4_wide); else 3-bit
  bool table;         // substitution scores from the plan's table (KArgs::sub); else match / mismatch
  bool profile;       // ... from the plan's profile instead (KArgs::prof): one 32-byte row of scores per ROW OF THE
                      // MATRIX, not per row code -- the lane's registers hold what they hold under a 32 x 32 table
  bool band;          // |i - j| <= band is accepted
  msa_walk walker;    // what walks its direction bytes
  int twin32;         // the same row over 5-bit codes, or MSA_ALG_NONE

  constexpr bool linear() const { return cell == CELL_LIN_FLOOR || cell == CELL_LIN || cell == CELL_LIN_PK16; }
  constexpr bool packed() const { return cell == CELL_LIN_PK16; }
  // Smith-Waterman: never masked -- columns outside [1, n] carry a virtual code -- and the best cell is the result
  constexpr bool local() const { return result == RES_BEST; }
  // a lane keeps the first maximum of its row, of any sign (from INT32_MIN)
  constexpr bool row_max() const { return result == RES_ROW_M || result == RES_ROW_M_COL || result == RES_BEST_ANY; }
  // ... the lane of row m alone
  constexpr bool row_m() const { return result == RES_ROW_M || result == RES_ROW_M_COL; }
};

// An id that IS another id with a band: that row with |i - j| <= band accepted, and a 32-code twin of its own.
constexpr msa_alg_info msa_alg_with_band(msa_alg_info t, int twin32) {
  t.band = true;
  t.twin32 = twin32;
  return t;
}

// clang-format off
constexpr msa_alg_info msa_alg_info_of(int alg) {
  constexpr msa_border RAMP = BORDER_RAMP, FREE = BORDER_FREE;
  switch (alg) {
    //                          nc cell            top   left  result         wide   table  prof   band   walker      twin32
    case MSA_ALG_SWL:   return {1, CELL_LIN_FLOOR, FREE, FREE, RES_BEST,      false, false, false, false, TB_NONE,    MSA_ALG_NONE};
    case MSA_ALG_SWL0:  return {1, CELL_LIN,       FREE, FREE, RES_BEST,      false, false, false, false, TB_NONE,    MSA_ALG_NONE};
    case MSA_ALG_SWLP:  return {1, CELL_LIN_PK16,  FREE, FREE, RES_BEST,      false, false, false, false, TB_NONE,    MSA_ALG_NONE};
    case MSA_ALG_SWA:   return {2, CELL_SWAFF,     FREE, FREE, RES_BEST,      false, false, false, false, TB_SW,      MSA_ALG_NONE};
    case MSA_ALG_SWS:   return {2, CELL_SWAFF,     FREE, FREE, RES_BEST,      false, true,  false, false, TB_SW,      MSA_ALG_SWS32};
    case MSA_ALG_SWS32: return {2, CELL_SWAFF,     FREE, FREE, RES_BEST,      true,  true,  false, false, TB_SW,      MSA_ALG_NONE};
    case MSA_ALG_NWA:   return {2, CELL_GOTOH,     RAMP, RAMP, RES_FINAL,     false, true,  false, true,  TB_NW,      MSA_ALG_NWA32};
    case MSA_ALG_NWA32: return {2, CELL_GOTOH,     RAMP, RAMP, RES_FINAL,     true,  true,  false, true,  TB_NW,      MSA_ALG_NONE};
    case MSA_ALG_FIT:   return {2, CELL_GOTOH,     FREE, RAMP, RES_ROW_M,     false, true,  false, false, TB_FIT,     MSA_ALG_FIT32};
    case MSA_ALG_FIT32: return {2, CELL_GOTOH,     FREE, RAMP, RES_ROW_M,     true,  true,  false, false, TB_FIT,     MSA_ALG_NONE};
    case MSA_ALG_OVL:   return {2, CELL_GOTOH,     FREE, FREE, RES_ROW_M_COL, false, true,  false, false, TB_FIT,     MSA_ALG_OVL32};
    case MSA_ALG_OVL32: return {2, CELL_GOTOH,     FREE, FREE, RES_ROW_M_COL, true,  true,  false, false, TB_FIT,     MSA_ALG_NONE};
    case MSA_ALG_EXT:   return {2, CELL_GOTOH,     RAMP, RAMP, RES_BEST_ANY,  false, true,  false, false, TB_FIT,     MSA_ALG_EXT32};
    case MSA_ALG_EXT32: return {2, CELL_GOTOH,     RAMP, RAMP, RES_BEST_ANY,  true,  true,  false, false, TB_FIT,     MSA_ALG_NONE};
    case MSA_ALG_REF:   return {3, CELL_REF3,      RAMP, RAMP, RES_FINAL,     false, false, false, false, TB_REF,     MSA_ALG_NONE};
    case MSA_ALG_REF1:  return {2, CELL_REF_TAG,   RAMP, RAMP, RES_FINAL,     false, false, false, false, TB_REF_TAG, MSA_ALG_NONE};
    case MSA_ALG_PART:  return {3, CELL_PART,      RAMP, RAMP, RES_FINAL,     false, false, false, false, TB_NONE,    MSA_ALG_NONE};
    case MSA_ALG_SWP:   return {2, CELL_SWAFF,     FREE, FREE, RES_BEST,      true,  true,  true,  false, TB_SW,      MSA_ALG_NONE};
    case MSA_ALG_NWP:   return {2, CELL_GOTOH,     RAMP, RAMP, RES_FINAL,     true,  true,  true,  false, TB_NW,      MSA_ALG_NONE};
    case MSA_ALG_FITP:  return {2, CELL_GOTOH,     FREE, RAMP, RES_ROW_M,     true,  true,  true,  false, TB_FIT,     MSA_ALG_NONE};
  }
  // the derived ids: a banded extension (MSA_NW_EXTEND_BAND) is the extension row, with a band -- the banded global
  // kernel's cell, borders, edge fix-ups and bytes under the extension's tracker, result rule and walker
  if (alg == MSA_ALG_EXTB) return msa_alg_with_band(msa_alg_info_of(MSA_ALG_EXT), MSA_ALG_EXTB32);
  if (alg == MSA_ALG_EXTB32) return msa_alg_with_band(msa_alg_info_of(MSA_ALG_EXT32), MSA_ALG_NONE);
  return {0, CELL_PART, RAMP, RAMP, RES_FINAL, false, false, false, false, TB_NONE, MSA_ALG_NONE};  // no such id
}
// clang-format on

// ---- the table checks itself -------------------------------------------------------------------------------------
namespace msa_alg_check {
enum { NC = 1, CELL = 2, TOP = 4, LEFT = 8, RESULT = 16, WIDE = 32, TABLE = 64, BAND = 128, WALKER = 256, TWIN = 512,
       PROFILE = 1024 };
// the fields in which two ids differ
constexpr unsigned diff(int x, int y) {
  const msa_alg_info a = msa_alg_info_of(x), b = msa_alg_info_of(y);
  return (a.nc != b.nc ? NC : 0) | (a.cell != b.cell ? CELL : 0) | (a.top != b.top ? TOP : 0) |
         (a.left != b.left ? LEFT : 0) | (a.result != b.result ? RESULT : 0) | (a.wide != b.wide ? WIDE : 0) |
         (a.table != b.table ? TABLE : 0) | (a.band != b.band ? BAND : 0) | (a.walker != b.walker ? WALKER : 0) |
         (a.twin32 != b.twin32 ? TWIN : 0) | (a.profile != b.profile ? PROFILE : 0);
}
constexpr int nc_of_cell(msa_cell c) {
  return (c == CELL_REF3 || c == CELL_PART) ? 3 : (c == CELL_SWAFF || c == CELL_GOTOH || c == CELL_REF_TAG) ? 2 : 1;
}
// every id: nc agrees with the cell; its twin, if any, is itself but for the code width (and has no twin of its own);
// a profile row is a row of a plan-owned table over 5-bit codes
constexpr bool rows_ok() {
  for (int alg = 0; alg <= MSA_ALG_EXTB32; ++alg) {
    const msa_alg_info t = msa_alg_info_of(alg);
    if (t.nc != nc_of_cell(t.cell) || (t.wide && !t.table) || (t.profile && !t.wide)) return false;
    if (t.twin32 != MSA_ALG_NONE && (t.wide || diff(alg, t.twin32) != (WIDE | TWIN))) return false;
  }
  return true;
}
static_assert(rows_ok(), "nc / cell, or an X32 row that is not its X row over 5-bit codes");
static_assert(msa_alg_info_of(MSA_ALG_NWA).twin32 == MSA_ALG_NWA32 && msa_alg_info_of(MSA_ALG_FIT).twin32 == MSA_ALG_FIT32 &&
                  msa_alg_info_of(MSA_ALG_OVL).twin32 == MSA_ALG_OVL32 && msa_alg_info_of(MSA_ALG_EXT).twin32 == MSA_ALG_EXT32 &&
                  msa_alg_info_of(MSA_ALG_SWS).twin32 == MSA_ALG_SWS32,
              "every X32 id is its X row's twin");
// overlap is fit with the left border free too, and the last column's maximum beside row m's
static_assert(diff(MSA_ALG_OVL, MSA_ALG_FIT) == (LEFT | RESULT | TWIN), "OVL = FIT but for the left border and the result");
// extension is the unbanded global kernel with another result (its walk starts there: TB_FIT, not TB_NW)
static_assert(diff(MSA_ALG_EXT, MSA_ALG_NWA) == (RESULT | BAND | WALKER | TWIN), "EXT = unbanded NWA but for the result");
// a banded extension is the extension with a band, and so the banded global kernel with the extension's result
static_assert(diff(MSA_ALG_EXTB, MSA_ALG_EXT) == (BAND | TWIN) && diff(MSA_ALG_EXTB32, MSA_ALG_EXT32) == BAND,
              "EXTB = EXT with a band");
static_assert(diff(MSA_ALG_EXTB, MSA_ALG_NWA) == (RESULT | WALKER | TWIN) &&
                  diff(MSA_ALG_EXTB32, MSA_ALG_NWA32) == (RESULT | WALKER),
              "EXTB = banded NWA but for the result");
static_assert(msa_alg_info_of(MSA_ALG_EXTB).twin32 == MSA_ALG_EXTB32, "EXTB32 is EXTB's twin");
// scored local is SW affine under the plan's table
static_assert(diff(MSA_ALG_SWS, MSA_ALG_SWA) == (TABLE | TWIN), "SWS = SWA under a table");
// a profile id is a 32-code id whose 32 scores belong to the row of the matrix (the global one takes no band: its
// launch is the stripe kernel's, and nothing of a band's geometry is position-specific)
static_assert(diff(MSA_ALG_SWP, MSA_ALG_SWS32) == PROFILE, "SWP = SWS32 under a profile");
static_assert(diff(MSA_ALG_NWP, MSA_ALG_NWA32) == (PROFILE | BAND), "NWP = unbanded NWA32 under a profile");
static_assert(diff(MSA_ALG_FITP, MSA_ALG_FIT32) == PROFILE, "FITP = FIT32 under a profile");
}  // namespace msa_alg_check

/*
 * msa.h -- C-ABI of the MI355X-native pairwise-alignment library (libmsa.so).
 *
 * Plain pointers and sizes only (no torch / HIP types in the signatures; a
 * stream is passed as `void*` holding a hipStream_t, NULL = default stream).
 * Every function returns an msa_status (0 = OK, < 0 = error); nothing throws
 * across this boundary.  All compute runs in hand-written HIP kernels for
 * gfx950; there is no CPU fallback: without a usable GPU the calls return
 * MSA_ERR_NODEV.
 *
 * Reference interfaces each entry point replaces (D-2n/CSE305_Parallel_Sequence_Alignment):
 *   msa_main_alignment   int main_alignment_function(char*,char*,size_t,size_t,size_t,double,double)
 *                        alignment_algorithm/main_alignment.h:38, .cpp:353-410
 *                        (with OptimalAlignmentMapThread :11-22 and print_seq :32-55)
 *   msa_subproblem       class Subproblem ctor + compute_tables() + find_alignment()
 *                        alignment_algorithm/subproblem_alignment.h:36-74,
 *                        subproblem_alignment.cpp:329-355 (fill), :105-172 (traceback)
 *   msa_partial_partition findPartialBalancedPartitionParallel(...)
 *                        sequence_alignment/partial.h:41, partial.cpp:149-163
 *   msa_non_parallel_tables  Subproblem::non_parallel_tables(), subproblem_alignment.cpp:357-422
 *   msa_subproblem_f64   Subproblem ctor + compute_tables() in double for any g, h (:251-355)
 *   msa_subproblem_row   Subproblem::compute_row / *MapThread bodies (:212-327)
 *   msa_optimal_alignment optimal_alignment(...), main_alignment.h:34, main_alignment.cpp:158-351
 *   msa_main_alignment_partitioned  main_alignment_function with its commented-out
 *                        partition step (main_alignment.cpp:365,372) enabled
 *   msa_partial_tables   initializeTables/initializeReverseTables/fillTablesParallel/
 *                        fillReverseTablesParallel, partial.h:25-35, partial.cpp:13-79
 *   msa_partition_tables findPartitionParallel over caller tables, partial.h:37-39, partial.cpp:81-146
 *   msa_plan_*           device-resident batch / single-pair fills (build extension:
 *                        configs C2-C5 of BASELINE.json; no reference counterpart,
 *                        same cell recurrence family as subproblem_alignment.cpp:396-398)
 *   msa_nw_align, msa_plan_traceback_nw
 *                        banded global (Gotoh) alignment with its CIGAR (build extension:
 *                        MSA_NW_ALIGN plans write one direction byte per in-band cell, the
 *                        walk runs on the device; same recurrence as MSA_NW_BANDED, +1 on equal symbols
 *                        and 0 otherwise)
 *   msa_plan_create_scored, msa_nw_align_scored, msa_nw_align_batch_scored
 *                        the same alignment under match / mismatch scores or an 8 x 8 substitution
 *                        matrix over the symbol codes (build extension: MSA_NW_SCORED plans)
 *   msa_plan_traceback_batch, msa_sw_align_batch, msa_nw_align_batch
 *                        the walks of a whole batch plan in one launch, and batches of local / global
 *                        alignments with their CIGARs from host pointers (build extension: one wave per
 *                        walk over the bytes msa_plan_traceback / msa_plan_traceback_nw walk)
 *   msa_fit_align, msa_fit_align_batch
 *                        fit alignment: the whole query against the substring of the reference it fits
 *                        best, with the reference span and the CIGAR (build extension: MSA_NW_FIT plans --
 *                        a zero top border, the first maximum of row m found inside the fill kernel, and
 *                        the two global walks started at that cell)
 *   msa_overlap_align, msa_overlap_align_batch, msa_overlap_align32, msa_overlap_align_batch32
 *                        overlap ("dovetail", "ends-free") alignment: a suffix of one sequence against a prefix
 *                        of the other, or one inside the other (build extension: MSA_NW_OVERLAP plans)
 *   msa_extend_align, msa_extend_align_batch, msa_extend_align32, msa_extend_align_batch32
 *                        extension alignment (anchored start, free end: what a seed-and-extend pipeline runs on
 *                        each flank of a seed): the best-scoring pair of prefixes, with the end-to-end score
 *                        beside it (build extension: MSA_NW_EXTEND plans)
 *   msa_extend_align_banded, msa_extend_align_batch_banded, msa_extend_align_banded32,
 *   msa_extend_align_batch_banded32, msa_extend_band_clip
 *                        the same inside a band |i - j| <= band, the work bounded by m, n and the band alone (build
 *                        extension: MSA_NW_EXTEND_BAND plans -- the banded global kernel's cells and edge phases
 *                        under the extension's end-cell tracker; the clip rule that stands for |m - n| <= band)
 *   msa_extend_align_xdrop, msa_extend_align_batch_xdrop, msa_extend_align_xdrop32,
 *   msa_extend_align_batch_xdrop32, msa_xdrop_extend_run, msa_xdrop_extend_walk
 *                        the banded extension with X-drop termination: the fill stops once the last two
 *                        anti-diagonals fall more than xdrop below the best score (build extension: a kernel family
 *                        of its own, one wave per pair, anti-diagonal by anti-diagonal; not a plan kind)
 *   msa_xdrop_flank_run, msa_seed_align, msa_seed_align_batch, msa_seed_align32, msa_seed_align_batch32
 *                        seed extension: both flanks of a seed in one call, the alignment through the seed (build
 *                        extension: the X-drop fill with a reading direction per pair, so a left flank is read
 *                        backwards in place from the uploaded buffers)
 *   msa_plan_create_scored32, msa_nw_align_scored32, msa_nw_align_batch_scored32, msa_fit_align32,
 *   msa_fit_align_batch32
 *                        MSA_NW_SCORED and MSA_NW_FIT over alphabets of up to 32 symbols (proteins, IUPAC DNA):
 *                        5-bit codes under a 32 x 32 int8 substitution table (build extension: stripe kernel
 *                        instantiations of their own, whose lanes hold a 32-byte row of the table and look four
 *                        scores up with seven v_perm_b32)
 *   msa_sw_align_scored, msa_sw_align_batch_scored, msa_sw_align_scored32, msa_sw_align_batch_scored32
 *                        local (Smith-Waterman) alignment under an int8 substitution matrix over up to 7 symbols,
 *                        or 31 over 5-bit codes (build extension: MSA_SW_SCORED plans -- the stripe kernel's
 *                        SW-affine cell with its score from the plan's table, the highest code kept as the
 *                        out-of-matrix sentinel; msa_plan_traceback and msa_plan_traceback_batch walk them)
 */
#ifndef MSA_H
#define MSA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------ */
typedef enum msa_status {
  MSA_OK = 0,
  MSA_ERR_ARG = -1,          /* bad argument (size 0 where the path needs >0, NULL, ...) */
  MSA_ERR_ALPHABET = -2,     /* more than 8 distinct symbols in a pair, or a symbol outside the caller's alphabet */
  MSA_ERR_HIP = -3,          /* a HIP runtime call failed */
  MSA_ERR_NODEV = -4,        /* no gfx950 device visible */
  MSA_ERR_UNSUPPORTED = -5,  /* e.g. non-integral g/h (the GPU path is exact int32) */
  MSA_ERR_TIMEOUT = -6,      /* a cross-workgroup wait exceeded its bound */
  MSA_ERR_NOMEM = -7,
  MSA_ERR_CAPACITY = -8,     /* caller buffer too small */
  MSA_ERR_NOMATCH = -9       /* traceback found no predecessor (cannot happen for integral g,h) */
} msa_status;

const char* msa_status_string(int status);
int msa_version(void);
/* number of usable gfx950 devices */
int msa_device_count(int* count);

/* Admission control of the host-pointer entry points (msa_main_alignment, msa_subproblem,
 * msa_partial_*, msa_sw_align, msa_optimal_alignment's subproblems).  The reference's callers
 * run main_alignment_function from hardware_concurrency threads at once on whole sequences
 * (test_functions/testing.cpp:269-280 and :352-358, calls at :261 and :345); every call here
 * reserves its estimated device footprint against a per-device budget before allocating and
 * waits (FIFO) until it fits, instead of failing with MSA_ERR_NOMEM.  A call larger than the
 * budget runs alone.  Budget: env MSA_DEVICE_BUDGET_MB, else 90% of device memory;
 * msa_set_device_budget(bytes) sets it for the current device (0 = back to the default).
 * msa_device_budget_info: out5 = {budget, bytes admitted now, peak admitted bytes since the
 * last set, calls that had to wait, calls admitted}. */
int msa_set_device_budget(int64_t bytes);
int msa_device_budget_info(int64_t* out5);
/* Memory held on the current device: out4 = {bytes admitted now, idle cached plans of the
 * reference walk (footprint estimate), free blocks of the device pool, admissions that released
 * the idle ones first}.  An admission that would put admitted + idle bytes over the budget first
 * destroys the idle cached plans and frees the pool's blocks.  Plans created directly through
 * msa_plan_create (the device-resident API below) are the caller's and are not admitted. */
int msa_device_memory_info(int64_t* out4);

/* Node of an alignment path: the reference's `align` struct
 * (subproblem_alignment.h:8-13) without the `next` pointer. */
typedef struct msa_node {
  uint64_t i;
  uint64_t j;
  int32_t t;
  int32_t pad;
} msa_node;

/* ---- reference-compatible host-pointer entry points ---------------------
 * Character arrays follow the reference's conventions: A1/B1 are 1-based
 * (A1[0] never read), compared for equality only. */

/* main_alignment_function: writes the exact stdout text the reference prints
 * ("bp1".."bp4" then print_seq's two lines) into `text` (NUL-terminated),
 * *text_len = its length.  *score = max(T1,T2,T3)[m][n] (not exposed by the
 * reference; returned for convenience).  p only sets the reference's thread
 * count and is accepted for signature parity. */
int msa_main_alignment(const char* A1, const char* B1, size_t m, size_t n, size_t p, double g, double h,
                       char* text, size_t text_cap, size_t* text_len, double* score);

/* Subproblem(A1,B1,m,n,idA,idB,p,start,end,g,h) -> compute_tables(), and when
 * nodes != NULL, find_alignment().  After the constructor's swap (m > n) the
 * tables are (m'+1) x (n'+1), m' = min(m,n); T1/T2/T3 (each NULL or
 * (m'+1)*(n'+1) int32, row-major) receive the tables with INT32_MIN standing
 * for -infinity.  nodes[0..*n_nodes) = alignment_begin .. alignment_end;
 * *end_node = alignment_end; *invert = the constructor's swap flag. */
int msa_subproblem(const char* A1, const char* B1, size_t m, size_t n, size_t idA, size_t idB, int start_type,
                   int end_type, double g, double h, int32_t* T1, int32_t* T2, int32_t* T3, msa_node* nodes,
                   size_t nodes_cap, size_t* n_nodes, msa_node* end_node, int* invert);

/* Subproblem::non_parallel_tables (subproblem_alignment.cpp:357-422): the
 * tables of msa_subproblem printed as the reference prints them ("T1:" then
 * one line per row of "%lf " cells, -inf as "-inf"; then T2, T3) into `text`
 * (NUL-terminated; *text_len = its length; text may be NULL to size it). */
int msa_non_parallel_tables(const char* A1, const char* B1, size_t m, size_t n, size_t idA, size_t idB,
                            int start_type, int end_type, double g, double h, char* text, size_t text_cap,
                            size_t* text_len);

/* The reference's tables in IEEE double for ANY g, h (the int32 entry points
 * need integral g, h): Subproblem ctor + compute_tables
 * (subproblem_alignment.h:36-74, .cpp:329-355) as its row sweep -- T1/T3
 * elementwise, T2 by omega + inclusive prefix max (:229-326) -- on the GPU,
 * with the same double operations in the same order (bit-identical cells).
 * T1/T2/T3: (m'+1) x (n'+1) row-major doubles (-inf as -infinity), m' =
 * min(m,n) after the constructor's swap (*invert).  m = n = 0 is MSA_ERR_ARG.
 * mode MSA_F64_NON_PARALLEL computes T2 by non_parallel_tables' direct
 * recurrence (:398) instead -- the same values for integral g, h; for others
 * the two forms round differently, and each mode matches its reference twin. */
enum { MSA_F64_COMPUTE_TABLES = 0, MSA_F64_NON_PARALLEL = 1 };
int msa_subproblem_f64(const char* A1, const char* B1, size_t m, size_t n, size_t idA, size_t idB, int start_type,
                       double g, double h, int mode, double* T1, double* T2, double* T3, int* invert);

/* One step of the reference's row sweep on the GPU (double, bit-identical),
 * for the source-compatible Subproblem's compute_row and MapThread bodies:
 *   MSA_ROW_ZERO  compute_row(0)                  subproblem_alignment.cpp:259-280 (cur = row 0)
 *   MSA_ROW_FULL  compute_row(i > 0)              :282-326 (up = row i-1, cur = row i; vec optional)
 *   MSA_ROW_FIRST ComputeFirstRowMapThread         :212-227 on cur, columns [start, end)
 *   MSA_ROW_13    ComputeRowMapThread13            :229-235 up -> cur T1/T3, columns [start, end)
 *   MSA_ROW_OMEGA ComputeOmegaMapThread            :237-242 cur T1/T3 -> vec[start, end)
 *   MSA_ROW_T2    ComputeRowMapThread2             :244-249 vec -> cur T2, columns [start, end)
 * A1/B1 with idA/idB as the Subproblem holds them (after its swap); rows are
 * n+1 doubles; column ranges need 1 <= start <= end <= n+1. */
enum { MSA_ROW_FIRST = 1, MSA_ROW_13 = 2, MSA_ROW_OMEGA = 4, MSA_ROW_T2 = 8, MSA_ROW_ZERO = 16, MSA_ROW_FULL = 32 };
int msa_subproblem_row(int part, const char* A1, const char* B1, size_t idA, size_t idB, size_t n, size_t i,
                       int start_type, double g, double h, size_t start, size_t end, const double* up1,
                       const double* up2, const double* up3, double* cur1, double* cur2, double* cur3, double* vec);

/* optimal_alignment(A, B, partial_bp, m, n, p, g, h) (main_alignment.h:34,
 * main_alignment.cpp:202-351): solves the subproblems between consecutive
 * partition points bp[k] -> bp[k+1] (start type bp[k].t, end type -bp[k+1].t)
 * on the GPU, concurrently, in the reference's selection (with 2 or 3
 * subproblems only subproblem 0 is solved, :237-279), stitches their node
 * lists as :344-348 does (the link into the last subproblem is never made) and
 * writes the stdout text: "bp1".."bp4" per solved subproblem, then print_seq's
 * two lines.  flags = MSA_OPT_FIX_ALL solves and links every subproblem.
 * path (may be NULL) receives the stitched node list.  p only sizes the
 * reference's thread counts (omega / ParallelPrefix / assign_processors,
 * :158-200) and is accepted for signature parity.  Partition points must be
 * non-decreasing in i and j and inside [0,m] x [0,n]; a 0 x 0 subproblem is
 * MSA_ERR_ARG (the reference crashes on both). */
enum { MSA_OPT_FIX_ALL = 1 };
int msa_optimal_alignment(const char* A1, const char* B1, size_t m, size_t n, size_t p, double g, double h,
                          const msa_node* bp, size_t n_bp, int flags, char* text, size_t text_cap, size_t* text_len,
                          msa_node* path, size_t path_cap, size_t* n_path);

/* main_alignment_function with the partition step the reference leaves
 * commented out (main_alignment.cpp:365,372): the GPU partition
 * findPartialBalancedPartitionParallel(A1+1, B1+1, m, n, p, g, h, -1, -1)
 * (partial.cpp reads A[i-1], so it gets the 0-based view) feeding
 * msa_optimal_alignment.  Same text contract as msa_main_alignment. */
int msa_main_alignment_partitioned(const char* A1, const char* B1, size_t m, size_t n, size_t p, double g,
                                   double h, int flags, char* text, size_t text_cap, size_t* text_len);

/* findPartialBalancedPartitionParallel (partial.cpp:149-163), int32 wrap
 * semantics; A0/B0 are 0-based (partial.cpp reads A[i-1]).  out receives the
 * p+1 sorted partition points. */
int msa_partial_partition(const char* A0, const char* B0, size_t m, size_t n, size_t p, double g, double h,
                          int start_type, int end_type, msa_node* out, size_t cap, size_t* n_out);

/* The six int32 tables partial.cpp builds: T* (m+1)x(n+1), R* (m+2)x(n+2),
 * row-major; any pointer may be NULL. */
int msa_partial_tables(const char* A0, const char* B0, size_t m, size_t n, double g, double h, int start_type,
                       int end_type, int32_t* T1, int32_t* T2, int32_t* T3, int32_t* R1, int32_t* R2, int32_t* R3);

/* findPartitionParallel(T1, T2, T3, TR1, TR2, TR3, m, n, p, h) (partial.h:37-39,
 * partial.cpp:81-146) over tables the caller already holds: T* (m+1)x(n+1) and
 * TR* (m+2)x(n+2) int32, row-major, as partial.cpp's own fills leave them.  The
 * band maxima run on the GPU (int32 wrap, first maximum in the reference's scan
 * order); out receives the p+1 points sorted as partial.cpp:141-143. */
int msa_partition_tables(const int32_t* T1, const int32_t* T2, const int32_t* T3, const int32_t* R1,
                         const int32_t* R2, const int32_t* R3, size_t m, size_t n, size_t p, double h,
                         msa_node* out, size_t cap, size_t* n_out);

/* ---- device-resident plans (configs C2-C5) --------------------------------
 * A plan owns the device scratch for one shape of work.  msa_plan_create
 * picks the kernel family from the description (msa_plan_launch_info reports
 * it): the stripe kernel (a batch, a small batch split into items, or one
 * pair), the flow kernels (one SW-linear pair; SW-affine / Gotoh with
 * direction bytes; pass 2 inside the launch or as a launch behind it), cflow
 * (packed score-only couples) or the band kernel (one banded pair, exact or
 * in chunks with the exact launch as fallback).  Running the plan stages the
 * column codes, launches that family and a tiny per-pair reduction on
 * `stream` (no allocation, no host sync inside msa_plan_run).  Inputs are
 * uint8 codes in [0,8) ([0,32) for msa_plan_create_scored32's plans) already in device memory (see msa_encode_pair for the
 * host-side code map); the
 * Smith-Waterman algorithms reserve code 7 (out-of-matrix sentinel), so their
 * inputs use codes 0..6 (MSA_SW_SCORED over 5-bit codes: code 31, inputs 0..30). */
typedef enum msa_alg_e {
  MSA_SW_LINEAR = 0,  /* Smith-Waterman, linear gap (gap_open == gap_extend used) */
  MSA_SW_AFFINE = 1,  /* Smith-Waterman, affine gap */
  MSA_NW_BANDED = 2,  /* reference Gotoh (g=gap_extend, h=gap_open-gap_extend), start type -1, optional band */
  MSA_REF_GOTOH = 3,  /* reference Gotoh T1/T2/T3, any start type, exact -inf */
  MSA_PARTIAL = 4,    /* partial.cpp forward Gotoh, int32 wrap */
  MSA_NW_ALIGN = 5,   /* MSA_NW_BANDED's recurrence with one direction byte per cell (MSA_CELLS_DIR only,
                         match = 1, mismatch = 0; walked by msa_plan_traceback_nw) */
  MSA_NW_SCORED = 6,  /* MSA_NW_ALIGN's recurrence, band rule, borders, tie order and direction byte with
                         f(i,j) = S[code of A_i][code of B_j]: S from match / mismatch, or an 8 x 8 table
                         (msa_plan_create_scored); MSA_CELLS_DIR (walked by msa_plan_traceback_nw /
                         msa_plan_traceback_batch) or MSA_CELLS_NONE (the score only) */
  MSA_NW_FIT = 7,     /* fit ("glocal", "semi-global", "infix") alignment: all of A against a substring of B that
                         the alignment chooses, MSA_NW_SCORED's cells under a zero top border; the contract is
                         at msa_fit_align below.  band = -1, MSA_CELLS_DIR or MSA_CELLS_NONE */
  MSA_SW_SCORED = 8,  /* MSA_SW_AFFINE's recurrence with f(i,j) = S[code of A_i][code of B_j]: the same zero floor,
                         borders, direction byte (h == 0 -> 0, then diagonal, E, F; bits 2 / 3 "open wins a tie"), end
                         cell (first maximum, row-major) and walk.  S from match / mismatch, or a table
                         (msa_plan_create_scored: 8 x 8, inputs are codes 0..6; msa_plan_create_scored32: 32 x 32,
                         codes 0..30 -- the highest code is the out-of-matrix sentinel's).  The contract is at
                         msa_plan_create_scored below */
  MSA_NW_OVERLAP = 9, /* overlap ("dovetail", "ends-free") alignment: MSA_NW_FIT's cells under zero borders on the top
                         AND the left, ending anywhere on the last row or the last column; the contract is at
                         msa_overlap_align below.  band = -1, MSA_CELLS_DIR or MSA_CELLS_NONE */
  MSA_NW_EXTEND = 10, /* extension alignment: an unbanded MSA_NW_SCORED plan's cells, borders and bytes, ending at the
                         first maximum over all interior cells (the best pair of prefixes) or nowhere; the contract is
                         at msa_extend_align below.  band = -1, MSA_CELLS_DIR or MSA_CELLS_NONE */
  MSA_NW_EXTEND_BAND = 11 /* extension alignment inside a band: a BANDED MSA_NW_SCORED plan's cells, borders and bytes,
                         ending at the first maximum over the in-band interior cells or nowhere; the contract is at
                         msa_extend_align_banded below.  band >= 0 and |m - n| <= band (msa_extend_band_clip),
                         MSA_CELLS_DIR or MSA_CELLS_NONE */
} msa_alg_e;

typedef enum msa_out_e { MSA_CELLS_NONE = 0, MSA_CELLS_H = 1, MSA_CELLS_DIR = 2, MSA_CELLS_TAB = 3 } msa_out_e;

typedef struct msa_plan_desc {
  int32_t alg;         /* msa_alg_e */
  int32_t cells;       /* msa_out_e */
  int32_t match, mismatch;
  int32_t gap_open;    /* SW: cost of the first gap char; Gotoh: g + h */
  int32_t gap_extend;  /* SW: each further gap char; Gotoh: g */
  int32_t start_type;  /* MSA_REF_GOTOH / MSA_PARTIAL */
  int32_t band;        /* MSA_NW_BANDED / MSA_NW_ALIGN: |i-j| <= band, -1 = none */
  int32_t track_end;   /* SW: also report the end cell (first max, row-major) */
  int32_t single;      /* 1: one pair spread over many workgroups; 0: one workgroup per pair */
  int64_t n_pairs;
  const int64_t* m;    /* host arrays, n_pairs each */
  const int64_t* n;
  const int64_t* a_off; /* offsets of each pair's row / column codes in the device arrays */
  const int64_t* b_off;
} msa_plan_desc;

typedef struct msa_pair_result {
  int32_t score;
  int32_t status;        /* 0, or -1: this run's row-m stripe left no final state (every run of a plan, not only
                            its first: the flag is cleared once it has been reported) */
  int64_t end_i, end_j;  /* SW: end cell; Gotoh: (m, n); MSA_NW_FIT: (m, first column of row m's maximum);
                            MSA_NW_OVERLAP: the end cell on row m or column n, or (m, 0) with score 0;
                            MSA_NW_EXTEND: the first maximum over the interior, or (0, 0) with score 0;
                            MSA_NW_EXTEND_BAND: ... over the in-band interior */
  int32_t fin[3];        /* Gotoh: state at (m, n) (T1,T2,T3 / H,E,F); MSA_NW_FIT: the same cell's (H,E,F), which
                            is not part of that algorithm's result; MSA_NW_EXTEND: the same, and part of the
                            result -- fin[0] = H(m, n) is the end-to-end (global) score */
  int32_t pad;
} msa_pair_result;

typedef struct msa_plan msa_plan;

int msa_plan_create(const msa_plan_desc* desc, msa_plan** plan);
/* msa_plan_create with a substitution table for MSA_NW_SCORED: sub = 64 scores, row-major sub[8*a + b] = the
 * score of A's code a against B's code b (it need not be symmetric).  sub == NULL: msa_plan_create (an
 * MSA_NW_SCORED plan then scores desc->match on the diagonal, desc->mismatch elsewhere).  A non-NULL sub with
 * any other algorithm is MSA_ERR_UNSUPPORTED.  MSA_NW_SCORED needs every score in [-128, 127], gap_extend >= 0,
 * gap_open >= gap_extend, MSA_CELLS_NONE or MSA_CELLS_DIR, and scores, gap costs and sizes inside the value
 * range of the int32 cells: with s = the largest |score|, g = gap_extend, G = gap_open,
 *     (s + 2 G + 2 g) (m + n + 256) + (G - g) < 2^28
 * for every pair (the derivation is at check_ranges, msa_plan.inc); anything else is MSA_ERR_UNSUPPORTED.  The
 * band rule and its MSA_ERR_ARG are MSA_NW_ALIGN's.  MSA_NW_FIT takes a table (or NULL: match / mismatch) in the
 * same way and under the same inequality (its zero top border is within the bound); it is MSA_ERR_UNSUPPORTED
 * with any band but -1 and with cells other than MSA_CELLS_DIR / MSA_CELLS_NONE.  MSA_NW_OVERLAP: exactly
 * MSA_NW_FIT's rules and errors (its zero left border is within the bound too).  MSA_NW_EXTEND: the same rules
 * and errors again (its cells and borders are the unbanded MSA_NW_SCORED plan's: the same inequality).
 * MSA_NW_EXTEND_BAND: MSA_NW_SCORED's rules with a band REQUIRED -- band < 0 is MSA_ERR_UNSUPPORTED, |m - n| > band is
 * MSA_ERR_ARG (clip with msa_extend_band_clip first) -- under the same inequality; a profile is MSA_ERR_UNSUPPORTED.
 * MSA_SW_SCORED takes a table too (NULL: desc->match on the diagonal, desc->mismatch elsewhere, in [-128, 127]; the
 * results are then an MSA_SW_AFFINE plan's).  The kernels keep their out-of-matrix sentinel: code 7 is the virtual
 * column's, the inputs are codes 0..6 -- 7 symbols --, table entries with either index 7 are ignored, and the launch's
 * own copy carries the sentinel score in that column of every row.  Cells MSA_CELLS_DIR or MSA_CELLS_NONE, band -1,
 * gap_open >= 0, gap_extend >= 0 (MSA_SW_AFFINE's rule) and, with smax = max(0, the largest entry over codes 0..6),
 *     smax min(m, n) < 2^29
 * for every pair; anything else is MSA_ERR_UNSUPPORTED.  The plan always tracks its end cell (desc->track_end is
 * ignored): packed with the value when smax min(m, n) < 65536 and n + 512 < 32768 for every pair, else by
 * compare-select (msa_plan_format_info).  Every MSA_SW_SCORED plan launches the stripe kernel (msa_plan_launch_info
 * mode 0), one pair or a batch: no flow, cflow or split launch.  msa_plan_traceback (one pair) and
 * msa_plan_traceback_batch (no walk for a score <= 0) walk its direction bytes under their unchanged contracts;
 * msa_plan_traceback_nw and msa_plan_traceback_gotoh reject it with MSA_ERR_UNSUPPORTED.  A non-NULL sub with
 * MSA_SW_AFFINE stays MSA_ERR_UNSUPPORTED, and MSA_SW_AFFINE plans choose their kernels as before. */
int msa_plan_create_scored(const msa_plan_desc* desc, const int8_t* sub, msa_plan** plan);
/* MSA_NW_SCORED, MSA_NW_FIT, MSA_NW_OVERLAP, MSA_NW_EXTEND and MSA_NW_EXTEND_BAND over 5-bit codes: sub32 = 1,024 scores, row-major
 * sub32[32*a + b] = the score of A's code a against B's code b.  The inputs of msa_plan_run are codes in [0, 32).  desc->alg must be one of
 * those five (anything else but MSA_SW_SCORED, below: MSA_ERR_UNSUPPORTED); sub32 == NULL is MSA_ERR_ARG.  Cells, band and gap rules, the
 * value-range inequality (s = the largest |score| of the 1,024) and their errors are msa_plan_create_scored's.
 * Such a plan always launches the stripe kernel (msa_plan_launch_info mode 0): one pair, a batch, any band (a banded
 * single pair runs the exact masked stripe launch).  msa_plan_format_info reports it in its fourth word;
 * msa_plan_traceback_nw and msa_plan_traceback_batch walk its direction bytes as they walk an 8-code plan's.
 * MSA_SW_SCORED is accepted too, under msa_plan_create_scored's rules for it with 31 in place of 7: code 31 is the
 * virtual column's, the inputs are codes 0..30 -- 31 symbols --, entries with either index 31 are ignored, smax is
 * taken over codes 0..30; msa_plan_traceback and msa_plan_traceback_batch walk it. */
int msa_plan_create_scored32(const msa_plan_desc* desc, const int8_t* sub32, msa_plan** plan);
/* MSA_SW_SCORED, MSA_NW_SCORED and MSA_NW_FIT under a position-specific score profile (a PSSM) in place of a table:
 * f(i,j) = prof[32 r + code of B_j], r the profile position of row i -- the score no longer depends on a symbol of
 * A, there is no A.  prof: host memory, prof_rows rows of 32 int8, row r column c = the score of profile position r
 * against column code c; the plan makes its own device copy and owns it, as it owns a table's.  Pair p's rows 1..m[p]
 * are profile rows desc->a_off[p] .. desc->a_off[p] + m[p] - 1; many pairs may name the same rows (a search: a_off
 * all 0).  prof == NULL, prof_rows < 1, a negative a_off[p] or a_off[p] + m[p] > prof_rows: MSA_ERR_ARG.  Any other
 * desc->alg: MSA_ERR_UNSUPPORTED, and so is any band but -1, for all three.  desc->match and desc->mismatch are
 * ignored.  Cells (MSA_CELLS_DIR or MSA_CELLS_NONE), the gap rules, the value-range inequalities, a local plan's
 * end-cell format rule and all their errors are msa_plan_create_scored32's for the same alg, with s = the largest
 * |entry| of the whole profile and smax = max(0, the largest entry over columns 0..30).  A local plan keeps code 31 as
 * the out-of-matrix sentinel: its inputs are codes 0..30 and column 31 of the caller's rows is ignored (the device
 * copy carries the sentinel score there); global and fit plans take codes 0..31.
 * msa_plan_run ignores dA (it may be NULL); dB is as for the 32-code plans.  Such a plan always launches the stripe
 * kernel (msa_plan_launch_info mode 0), one pair or a batch: each lane loads its row's 32 bytes itself, and from there
 * on the fill, the direction bytes and the results are a 32-code plan's -- for the profile whose row r is row
 * code(A_r) of a 32 x 32 table, byte for byte that table plan's.  msa_plan_traceback (local), msa_plan_traceback_nw
 * (global, fit) and msa_plan_traceback_batch walk it under their unchanged contracts.  msa_plan_format_info reports
 * it in bit 1 of its fourth word.
 * Not offered: overlap and extension profiles, a band, profiles over 3-bit codes, position-specific gap costs and
 * profile-profile alignment. */
int msa_plan_create_profile(const msa_plan_desc* desc, const int8_t* prof, int64_t prof_rows, msa_plan** plan);
void msa_plan_destroy(msa_plan* plan);
/* Elements (int32 for H/TAB planes, bytes for DIR) the per-cell output needs. */
int msa_plan_cells_size(const msa_plan* plan, int64_t* elems);
/* Launch on `stream`.  dA/dB: device code arrays (dA is ignored by a profile plan and may be NULL for it).
 * cells0..2: device output (H: cells0; DIR: cells0 as uint8; TAB: three planes), may be NULL for NONE. */
int msa_plan_run(msa_plan* plan, const uint8_t* dA, const uint8_t* dB, void* cells0, void* cells1, void* cells2,
                 void* stream);
/* Copy per-pair results to the host (synchronizes `stream`).  Returns
 * MSA_ERR_TIMEOUT if any run since the plan was created (or since the last
 * msa_plan_clear_error) had a kernel wait hit its spin limit: the plan's error
 * word is sticky, so one check after many runs covers all of them. */
int msa_plan_results(msa_plan* plan, msa_pair_result* out, void* stream);
/* How the last run was computed: out4 = {launch mode (0 stripe kernel, 1 two-pass
 * flow kernel, 2 chunked banded), chunks, converged (chunked: 1 = every chunk
 * converged and the cells came from the chunk launch, 0 = the exact single-mode
 * launch recomputed them; -1 otherwise), warm-up stripes per chunk | 1 << 16 when
 * chunks >= 1 wrote int16 cells widened by the chunk constants' add}.
 * Synchronizes `stream` for mode 2. */
int msa_plan_run_info(msa_plan* plan, int32_t* out4, void* stream);
/* How the plan launches (for tests and tools): out8 = {mode: 0 stripe_kernel (batch), 1 flow_kernel
 * (single pair, two-pass), 2 chunked banded stripe_kernel, 3 split batch (every pair split into items
 * over several CUs), 4 band_kernel exact chain, 5 band_kernel chunked, 6 cflow_kernel (packed score-only
 * batch as flag-synchronised chains); workgroups of the main launch;
 * threads per workgroup; dynamic LDS bytes; flow pass-1 workgroups; workgroups of the separate pass-2
 * launch (flow_fill_kernel, long pairs; 0 = pass 2 runs inside the main launch); rows per lane;
 * items}. */
int msa_plan_launch_info(const msa_plan* plan, int32_t* out8);
/* The number formats the plan chose (read-only; for tests and tools): out4 = {value format: 0 int32, 1 packed
 * int16 couples (two score-only SW-linear pairs per lane), 2 the x4 tagged values of the reference's Gotoh
 * (start type -1); end-cell tracking: 0 none, 1 compare-select on (value, position), 2 the first maximum's
 * step packed with the value into one int; 1 if the chunks of a chunked banded plan write int16 cells;
 * bit 0: a plan over 5-bit codes (msa_plan_create_scored32, msa_plan_create_profile), bit 1: a profile plan
 * (msa_plan_create_profile); 0 for every other plan}. */
int msa_plan_format_info(const msa_plan* plan, int32_t* out4);
/* The sticky error word (0 = no error; else the kernel site code), synchronizes. */
int msa_plan_error(msa_plan* plan, int* code, void* stream);
/* Reset the sticky error word (stream-ordered). */
int msa_plan_clear_error(msa_plan* plan, void* stream);
/* Per-pair scores of the last run into a device int32 array of n_pairs
 * (device-to-device copy on `stream`, no host sync): the input of a score
 * all-gather across ranks. */
int msa_plan_scores(msa_plan* plan, int32_t* d_scores, void* stream);
/* Per-stripe metadata (cs, phases ...) of the last run: 12 int32 per stripe. */
int msa_plan_stripe_meta(msa_plan* plan, int32_t* out, int64_t cap_stripes, void* stream);
int64_t msa_plan_stripes(const msa_plan* plan);
/* Layout of one pair's cells in the skewed output: out4 = {first stripe index
 * in the meta array, pmax (16-step blocks per stripe), element offset of the
 * pair's block, DP steps per kernel phase | R << 16}.  R = rows per lane
 * (0 means 1).  Cell (i, j) of stripe s = (i-1)/(64R), lane r = ((i-1)%(64R))/R,
 * row rho = (i-1)%R, step t = j - cs_s + r lives at element
 * out_off + ((s*pmax*4 + t/4)*R + rho)*256 + r*4 + t%4 (DIR bytes, R = 1:
 * (s*pmax + t/16)*1024 + r*16 + t%16), cs_s = meta[12*(stripe0+s)].  R = 2 only
 * for two-pass single-pair SW-linear H plans. */
int msa_plan_pair_layout(const msa_plan* plan, int64_t pair, int64_t* out4);
/* Smith-Waterman traceback ON THE DEVICE (msa_traceback.hip), for an
 * MSA_SW_AFFINE (with track_end) or MSA_SW_SCORED plan with MSA_CELLS_DIR after msa_plan_run on the same stream:
 * one workgroup (a walker wave, four stripe-group loader waves, an op decoder
 * wave) walks pair `pair`'s direction bytes dDir from the end cell the run
 * found (first maximum, row-major) and writes the ops end -> start into d_ops
 * ('M' diagonal, 'D' gap consuming B, 'I' gap consuming A; at most ops_cap,
 * m+n suffices) and d_info[8] = {n_ops, beg_i, beg_j, status, stripes
 * entered, groups staged on demand, s_memtime ticks of the walk, times the
 * walker waited for a loader} (beg = the first aligned cell, 1-based; status
 * 0, MSA_ERR_CAPACITY or MSA_ERR_TIMEOUT).  Asynchronous,
 * no host sync; tie order of the oracle's orc_sw. */
int msa_plan_traceback(msa_plan* plan, int64_t pair, const uint8_t* dDir, uint8_t* d_ops, int64_t ops_cap,
                       int64_t* d_info, void* stream);
/* Subproblem::find_alignment ON THE DEVICE (replaces the host walk over the
 * reference's T1/T2/T3 tables, subproblem_alignment.cpp:105-172) for an
 * MSA_REF_GOTOH plan with MSA_CELLS_DIR, after msa_plan_run on the same stream:
 * one wave starts at (m, n) in the table the reference's end rule picks for
 * end_type (:112-146, from the run's final state; end_type in {-3..-1, 1..3})
 * and walks the direction bytes until i == 0 or j == 0 (:147).  d_ops receives
 * one op per step, end -> start: the table the step leaves ('M' T1 / diagonal,
 * 'D' T2 / consumes B, 'I' T3 / consumes A; at most ops_cap, m+n suffices);
 * d_info[8] as msa_plan_traceback, with {n_ops, i+1, j+1, status} where (i, j)
 * is the border cell the walk stopped at and status 0, MSA_ERR_CAPACITY or
 * MSA_ERR_NOMATCH.  The reference's align nodes (coordinates, quirks Q1/Q2)
 * follow from the ops on the host in O(m+n) (msa_main_alignment does this). */
int msa_plan_traceback_gotoh(msa_plan* plan, int64_t pair, int end_type, const uint8_t* dDir, uint8_t* d_ops,
                             int64_t ops_cap, int64_t* d_info, void* stream);
/* Global (Needleman-Wunsch / Gotoh) traceback ON THE DEVICE for an MSA_NW_ALIGN plan (or an MSA_NW_SCORED
 * plan with MSA_CELLS_DIR), after
 * msa_plan_run on the same stream.  The plan computes MSA_NW_BANDED's recurrence (f = 1 on equal
 * codes else 0 -- MSA_NW_SCORED: the plan's table entry --, g = gap_extend, h = gap_open - gap_extend >= 0;
 * cells with |i - j| > band are -inf):
 *   E(i,j) = max(H(i,j-1) - (g+h), E(i,j-1) - g)      F(i,j) = max(H(i-1,j) - (g+h), F(i-1,j) - g)
 *   H(i,j) = max(H(i-1,j-1) + f, E(i,j), F(i,j))      score = H(m,n)
 * and writes one byte per cell (skewed stripe layout, msa_plan_pair_layout), in the SW-affine
 * format: bits 0-1 = 1 if H equals the diagonal term, else 2 if H equals E, else 3 (F); bit 2 set
 * iff E(i,j) == H(i,j-1) - (g+h) (a tie with the extension goes to "open"); bit 3 the same for F and
 * H(i-1,j).  Bits 2 / 3 mean nothing where E / F is -inf; bytes of cells outside the band mean nothing.
 * The walk (tie order of the oracle's orc_sw) starts at (m, n) in state H.  H: low bits 1 -> 'M',
 * to (i-1, j-1); 2 -> state E; 3 -> state F.  E: 'D', j--, back to H if bit 2, else stay.  F: 'I',
 * i--, back to H if bit 3, else stay.  It stops as soon as i == 0 or j == 0; the rest of the
 * alignment is the border gap (i x 'I' or j x 'D'), which the caller appends.  d_ops receives the
 * ops end -> start (at most ops_cap; m+n suffices); d_info[8] as msa_plan_traceback_gotoh: {n_ops,
 * i+1, j+1, status, stripes entered, groups staged on demand, ticks, waits} with (i, j) the border
 * cell where the walk stopped and status 0 or MSA_ERR_CAPACITY.  Asynchronous, one walk per call
 * (msa_plan_traceback_batch walks every pair of a batch plan in one launch).  MSA_ERR_UNSUPPORTED for any plan that is not MSA_NW_ALIGN
 * or MSA_NW_SCORED with direction bytes; msa_plan_traceback and msa_plan_traceback_gotoh reject both.
 * An MSA_NW_FIT plan with direction bytes is walked too: the same walk, started at the pair's end cell (m, end_j)
 * from the run's result (an end cell outside the matrix -- the plan has not run -- is status MSA_ERR_ARG); the
 * caller appends only the i x 'I' border gap, and the stop column j is where the aligned substring begins.
 * An MSA_NW_OVERLAP plan with direction bytes likewise, from its end cell (end_i, end_j) on the last row or column;
 * nothing is appended, and the stop cell (i, j) is where the alignment begins.  Its empty overlap -- end cell (m, 0)
 * -- is no walk: n_ops 0, stop cell (m, 0), status 0.  msa_plan_traceback and msa_plan_traceback_gotoh reject it.
 * An MSA_NW_EXTEND plan with direction bytes likewise, from its end cell (end_i, end_j) anywhere in the interior (an
 * end cell outside the matrix -- the plan has not run -- is status MSA_ERR_ARG); the caller appends the global
 * border gap (i x 'I', else j x 'D': the start is anchored at (0, 0)).  Its empty extension -- end cell (0, 0) -- is
 * no walk: n_ops 0, stop cell (0, 0), status 0.  msa_plan_traceback and msa_plan_traceback_gotoh reject it. */
int msa_plan_traceback_nw(msa_plan* plan, int64_t pair, const uint8_t* dDir, uint8_t* d_ops, int64_t ops_cap,
                          int64_t* d_info, void* stream);
/* Every pair's traceback ON THE DEVICE in ONE launch (msa_tbatch.hip), after msa_plan_run on the same
 * stream: one wave per pair, four walks per workgroup, each wave staging its own stripe groups and writing
 * its own ops (the single walkers above spend a six-wave workgroup on one long walk and take a launch
 * per pair).  Plans: MSA_SW_AFFINE with MSA_CELLS_DIR and track_end, or MSA_SW_SCORED with MSA_CELLS_DIR (msa_plan_traceback's walk, from each
 * pair's end cell; no walk for a score <= 0) or MSA_NW_ALIGN / MSA_NW_SCORED (msa_plan_traceback_nw's walk, from (m, n) to
 * the matrix border; the caller appends the border gap; MSA_NW_FIT: that walk from each pair's (m, end_j);
 * MSA_NW_OVERLAP: from each pair's (end_i, end_j), n_ops 0 for an empty overlap; MSA_NW_EXTEND: the same, n_ops 0 for
 * an empty extension, and the global border gap is the caller's to append), laid
 * out one row per lane with the stripe starts
 * in the stripe meta: the stripe kernel's batch, split-batch and single launches and the band kernel's.
 * MSA_ERR_UNSUPPORTED, before any launch, for the flow kernels' plans (msa_plan_launch_info mode 1: the
 * single walkers serve them) and for every other algorithm / cells combination (MSA_REF_GOTOH included);
 * MSA_ERR_ARG for a NULL pointer.  d_ops_off: DEVICE array of n_pairs + 1 non-decreasing byte offsets;
 * pair p's ops (end -> start, 'M' / 'D' / 'I' as above) go to d_ops + d_ops_off[p], at most
 * d_ops_off[p+1] - d_ops_off[p] of them (m + n suffices; any byte alignment); bytes outside a pair's n_ops
 * are not written.  d_info: 8 int64 per pair, {n_ops, i+1, j+1, status, stripes entered, groups staged,
 * s_memtime ticks of the walk, 0}; words 0-3 are the single walker's for that pair (SW: the first aligned
 * cell; NW: the border cell where the walk stopped, + 1; status 0, MSA_ERR_CAPACITY with the true n_ops,
 * MSA_ERR_NOMATCH, or MSA_ERR_TIMEOUT: every walk is bounded by m + n + 2 stripes + 8 stripe / group
 * changes, whatever bytes dDir holds).  Asynchronous: no allocation, no host sync. */
int msa_plan_traceback_batch(msa_plan* plan, const uint8_t* dDir, uint8_t* d_ops, const int64_t* d_ops_off,
                             int64_t* d_info, void* stream);
/* Order-independent digest of pair `pair`'s H cells (oracle orc_checksum_h). */
int msa_plan_checksum(msa_plan* plan, const int32_t* dH, int64_t pair, uint64_t* digest, void* stream);
/* Device time (ms) of the last msa_plan_run's stripe kernel, from HIP events
 * recorded on the run's stream (synchronizes).  MSA_ERR_ARG if that run had
 * timing off. */
int msa_plan_last_kernel_ms(msa_plan* plan, float* ms);
/* Record the timing events in msa_plan_run (default on); off saves two stream
 * commands per run. */
int msa_plan_set_timing(msa_plan* plan, int on);

/* Map the symbols of a pair to codes 0..7 (equality preserved, first-seen
 * order).  Returns MSA_ERR_ALPHABET for more than 8 distinct symbols. */
int msa_encode_pair(const char* A0, size_t m, const char* B0, size_t n, uint8_t* codesA, uint8_t* codesB);

/* Host-pointer Smith-Waterman (build extension): score, end cell (first max
 * in row-major order) and, when cigar != NULL, the traceback as a run-length
 * M/I/D string (I consumes A, D consumes B) with its start cell.  At most 7
 * distinct symbols (MSA_ERR_ALPHABET otherwise). */
int msa_sw_align(const char* A0, size_t m, const char* B0, size_t n, int32_t match, int32_t mismatch,
                 int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_i, int64_t* end_j,
                 int64_t* beg_i, int64_t* beg_j, char* cigar, size_t cigar_cap);

/* Host-pointer global alignment (build extension): the MSA_NW_ALIGN fill, msa_plan_traceback_nw's
 * walk and the border gap, as a run-length M/I/D string start -> end (I consumes A, D consumes B)
 * that consumes exactly m and n.  Scoring as MSA_NW_BANDED: +1 on equal symbols, 0 otherwise, a gap
 * of L costs (gap_open - gap_extend) + gap_extend * L; gap_open >= gap_extend >= 0, else
 * MSA_ERR_UNSUPPORTED.  band = -1: no band; band >= 0 needs |m - n| <= band (MSA_ERR_ARG).  At most
 * 8 distinct symbols (MSA_ERR_ALPHABET).  *score = H(m, n).  cigar == NULL: the score only (no
 * direction bytes are written).  The call is admitted against the device budget with the band's
 * footprint (~(2 band + 64) bytes per row), not the full matrix's. */
int msa_nw_align(const char* A0, size_t m, const char* B0, size_t n, int32_t gap_open, int32_t gap_extend,
                 int64_t band, int32_t* score, char* cigar, size_t cigar_cap);

/* Host-pointer batches (build extension): n_pairs local (msa_sw_align_batch) or global (msa_nw_align_batch)
 * alignments with their CIGARs.  Pair p is A[a_off[p] .. a_off[p] + m[p]) against B[b_off[p] .. b_off[p] +
 * n[p]), 0-based; ranges may overlap or coincide (many queries against one reference: b_off all 0, the
 * reference uploaded once).  A range outside [0, a_len) / [0, b_len), m[p] or n[p] < 1, n_pairs < 1 or a NULL
 * array: MSA_ERR_ARG.  ONE symbol map serves the whole call -- first-seen order over A[0..a_len), then
 * B[0..b_len) -- which is what lets pairs share a sequence; it is stricter than msa_sw_align's and
 * msa_nw_align's per-pair maps: at most 7 (SW) / 8 (NW) distinct symbols in the two buffers together, else
 * MSA_ERR_ALPHABET.  Scoring, the band rule (band >= 0 needs |m[p] - n[p]| <= band for every pair; a band >=
 * every max(m[p], n[p]) is no band) and the other errors are msa_sw_align's and msa_nw_align's.
 * score: n_pairs.  end_ij / beg_ij (SW; either may be NULL): 2 n_pairs, {i, j} per pair.  cigars receives the
 * NUL-terminated run-length strings back to back (start -> end, I consumes A, D consumes B; NW strings
 * consume exactly m[p] and n[p]), cigar_off[p] = the start of pair p's, cigar_off[n_pairs] = the bytes used;
 * cigar_off (n_pairs + 1) is required with cigars.  A cigars too small: MSA_ERR_CAPACITY with the needed size
 * in cigar_off[n_pairs].  cigars == NULL (SW: and beg_ij == NULL): scores (and SW end cells) only, from plans
 * without direction bytes.
 * Consecutive pairs run in chunks whose summed single-pair footprint estimates stay within a quarter of the
 * device budget (a larger pair is a chunk alone); a chunk is admitted once and is one upload, one batch plan,
 * one msa_plan_run, one msa_plan_traceback_batch and two downloads.  The first nonzero walk status or plan
 * error is the call's status. */
int msa_sw_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                       const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                       int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend,
                       int32_t* score, int64_t* end_ij, int64_t* beg_ij,
                       char* cigars, size_t cigar_cap, int64_t* cigar_off);
int msa_nw_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                       const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                       int32_t gap_open, int32_t gap_extend, int64_t band,
                       int32_t* score, char* cigars, size_t cigar_cap, int64_t* cigar_off);

/* msa_nw_align and msa_nw_align_batch under a substitution matrix (build extension: MSA_NW_SCORED plans).
 * alphabet: n_sym distinct bytes, 1 <= n_sym <= 8; a symbol's code is its index.  sub: n_sym x n_sym scores,
 * row-major, the row is A's symbol (sub[n_sym * a + b] scores alphabet[a] in A against alphabet[b] in B; it need
 * not be symmetric).  A duplicate in alphabet, n_sym outside 1..8, or a NULL alphabet or sub: MSA_ERR_ARG.  A
 * symbol of A or B that is not in alphabet: MSA_ERR_ALPHABET.  Scores and gap costs outside the plan's value
 * range (msa_plan_create_scored): MSA_ERR_UNSUPPORTED.  Everything else -- the gap and band rules, admission,
 * chunks of pairs, the border gap, the CIGAR format, MSA_ERR_CAPACITY, cigar(s) == NULL for the score(s) alone
 * -- is msa_nw_align's and msa_nw_align_batch's. */
int msa_nw_align_scored(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                        char* cigar, size_t cigar_cap);
int msa_nw_align_batch_scored(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                              int32_t gap_extend, int64_t band, int32_t* score, char* cigars, size_t cigar_cap,
                              int64_t* cigar_off);

/* Fit alignment (build extension: MSA_NW_FIT plans; other tools say "glocal", "semi-global" or "infix"): ALL of
 * the query A against a SUBSTRING of the reference B that the alignment chooses; reference symbols before and
 * after the substring are free.  The contract:
 *   Inputs: A (m >= 1) and B (n >= 1) as codes in [0, 8), all eight usable; a score table S as for
 *   MSA_NW_SCORED (8 x 8 int8, or match / mismatch); g = gap_extend >= 0, h = gap_open - gap_extend >= 0, a gap of
 *   length L costs h + g L.
 *     H(0, j) = 0  for 0 <= j <= n        E(0, j) = F(0, j) = -inf
 *     H(i, 0) = F(i, 0) = -h - g i        E(i, 0) = -inf                (1 <= i <= m: as the global plan)
 *     E, F, H of interior cells, the direction byte and every tie rule: msa_plan_traceback_nw's text above
 *     score = max over 1 <= j <= n of H(m, j);   end_j = the SMALLEST such j (the first maximum along row m)
 *   Column 0 is left out of the maximum: F(m, 1) >= H(0, 1) - h - g m = H(m, 0), so H(m, 1) >= H(m, 0) and the
 *   optimum over 1..n is the optimum over 0..n.
 *   The walk is msa_plan_traceback_nw's, started at (m, end_j) in state H; it stops as soon as i == 0 or j == 0,
 *   at the stop cell (i, j).  If i > 0 (the query overhangs the reference's start) the caller appends i x 'I'; no
 *   'D' is ever appended, and beg_j = j.  The alignment consumes all m symbols of A and B[beg_j, end_j) (0-based,
 *   half open); the CIGAR (start -> end, run-length M/I/D, I consumes A) consumes exactly m and end_j - beg_j.
 *   beg_j == end_j is legal: the best alignment inserts the whole query.
 *   A plan reports PairResult{score, status, end_i = m, end_j}; fin[] holds (H, E, F) at (m, n) as a global plan's
 *   does and is not part of this algorithm's result.
 *   Out of scope, each MSA_ERR_UNSUPPORTED at plan creation: any band other than -1 (|i - j| <= band means nothing
 *   here), cells other than MSA_CELLS_DIR / MSA_CELLS_NONE, free ends on A (those are MSA_NW_OVERLAP's, below, with
 *   all four ends free at once).  Such plans always run the stripe
 *   kernel (msa_plan_launch_info mode 0), one pair or a batch.
 * msa_fit_align / msa_fit_align_batch behave as msa_nw_align_scored / msa_nw_align_batch_scored (alphabet, matrix
 * and range errors; admission against the device budget, here with the full m x n bytes; chunks of consecutive
 * pairs within a quarter of the budget, each one upload, one plan, one msa_plan_run, one msa_plan_traceback_batch
 * and two downloads; a reference shared by every pair -- all b_off equal -- uploaded once; MSA_ERR_CAPACITY, the
 * batch with the needed size in cigar_off[n_pairs]; argument errors decided on the host before any device call),
 * without a band argument.  *score, *beg_j, *end_j (each may be NULL) / score (n_pairs), beg_end (2 n_pairs,
 * {beg_j, end_j} per pair, required).  cigar(s) == NULL: scores and end_j from plans without direction bytes,
 * beg_j = -1. */
int msa_fit_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                  const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_j,
                  int64_t* end_j, char* cigar, size_t cigar_cap);
int msa_fit_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                        const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                        const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                        int32_t gap_extend, int32_t* score, int64_t* beg_end /* 2 n_pairs: {beg_j, end_j} */,
                        char* cigars, size_t cigar_cap, int64_t* cigar_off);

/* Overlap alignment (build extension: MSA_NW_OVERLAP plans; other tools say "dovetail", "ends-free" or "semi-global
 * with all four ends free"): the best alignment of a SUFFIX of one sequence with a PREFIX of the other, or of one
 * sequence contained in the other.  The contract:
 *   Inputs: A (m >= 1) and B (n >= 1); a score table S as for MSA_NW_SCORED (int8, 8 x 8 or 32 x 32, or match /
 *   mismatch); g = gap_extend >= 0, h = gap_open - gap_extend >= 0, a gap of length L costs h + g L.
 *     H(0, j) = 0  (0 <= j <= n)      H(i, 0) = 0  (1 <= i <= m)
 *     E = F = -inf on both borders
 *     E, F, H of interior cells, the direction byte and every tie rule: msa_plan_traceback_nw's text above
 *     row candidates:    H(m, j), 1 <= j <= n;  best_r = their maximum, j_r the SMALLEST j attaining it
 *     column candidates: H(i, n), 1 <= i <= m;  best_c = their maximum, i_c the SMALLEST i attaining it
 *     best = max(best_r, best_c)
 *     end cell = (m, j_r) if best_r >= best_c, else (i_c, n)      (the last row wins a tie)
 *     if best <= 0: the empty overlap -- score 0, end cell (m, 0), no walk, empty CIGAR
 *     else:         score = best
 *   The walk is msa_plan_traceback_nw's, started at the end cell in state H; it stops as soon as i == 0 or j == 0,
 *   at the stop cell (i, j).  NOTHING is appended: both prefixes are free.
 *   The result is (score, a_beg = i, a_end = end_i, b_beg = j, b_end = end_j): A[a_beg, a_end) against
 *   B[b_beg, b_end), 0-based and half open, with a_beg == 0 or b_beg == 0, and a_end == m or b_end == n; the CIGAR
 *   (start -> end, run-length M/I/D, I consumes A) consumes exactly a_end - a_beg and b_end - b_beg.  The empty
 *   overlap is (0, m, m, 0, 0).
 *   A plan reports PairResult{score, status, end_i, end_j}; fin[] holds (H, E, F) at (m, n) as a fit plan's does
 *   and is not part of this algorithm's result.
 *   Out of scope, each MSA_ERR_UNSUPPORTED at plan creation: any band other than -1, cells other than
 *   MSA_CELLS_DIR / MSA_CELLS_NONE; which ends are free is not selectable (MSA_NW_FIT frees B's alone).  Such plans
 *   always run the stripe kernel (msa_plan_launch_info mode 0), one pair or a batch, never a split batch, and the
 *   value-range inequality of msa_plan_create_scored holds unchanged (zero borders are inside its bound).
 * The entries behave as msa_fit_align / msa_fit_align_batch and their *32 twins in everything else, in the order
 * documented there: argument, alphabet and range errors decided on the host; admission with the full m x n bytes;
 * chunks of consecutive pairs within a quarter of the budget; a B shared by every pair uploaded once;
 * MSA_ERR_CAPACITY, the batch with the needed size in cigar_off[n_pairs].  *score, beg_ij[2] = {a_beg, b_beg},
 * end_ij[2] = {a_end, b_end} (each may be NULL) / score (n_pairs), beg_ij and end_ij (2 n_pairs each, required).
 * cigar(s) == NULL: scores and end cells from plans without direction bytes, beg_ij = {-1, -1}. */
int msa_overlap_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                      const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                      int64_t* end_ij, char* cigar, size_t cigar_cap);
int msa_overlap_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                            const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                            const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                            int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij, char* cigars,
                            size_t cigar_cap, int64_t* cigar_off);
/* ... for alphabets of up to 32 symbols, as msa_fit_align32 is to msa_fit_align (9..32 symbols: MSA_ALG_OVL32 plans) */
int msa_overlap_align32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                        int64_t* end_ij, char* cigar, size_t cigar_cap);
int msa_overlap_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                              int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij, char* cigars,
                              size_t cigar_cap, int64_t* cigar_off);

/* Extension alignment (build extension: MSA_NW_EXTEND plans; BWA-MEM's and minimap2's "extz", BLAST's gapped
 * extension): the alignment STARTS at the first symbols of both sequences and may stop anywhere -- the best-scoring
 * pair of prefixes A[0, a_end) against B[0, b_end).  A caller with a seed hit runs it twice per seed: rightwards on the
 * two flanks, leftwards on the reversed ones.  The contract:
 *   Inputs: A (m >= 1) and B (n >= 1); a score table S as for MSA_NW_SCORED (int8, 8 x 8 or 32 x 32, or match /
 *   mismatch); g = gap_extend >= 0, h = gap_open - gap_extend >= 0, a gap of length L costs h + g L.
 *     H(0, 0) = 0    H(0, j) = E(0, j) = -h - g j  (1 <= j <= n)    H(i, 0) = F(i, 0) = -h - g i  (1 <= i <= m)
 *     E, F, H of interior cells, the direction byte and every tie rule: msa_plan_traceback_nw's text above -- exactly an
 *     unbanded MSA_NW_SCORED plan's, so the direction bytes of the two plans on one input are equal byte for byte
 *     (where that plan's bytes mean anything)
 *     best = max of H(i, j) over 1 <= i <= m, 1 <= j <= n
 *     end cell = the FIRST maximum in row-major order: the smallest i, then the smallest j (Smith-Waterman's rule)
 *     if best <= 0: the empty extension -- score 0, end cell (0, 0), no walk, empty CIGAR.  (Border cells are never
 *                   candidates: they are <= 0, and the empty extension stands for them)
 *     else:         score = best
 *   The walk is msa_plan_traceback_nw's, started at the end cell in state H; it stops as soon as i == 0 or j == 0, and
 *   the caller appends the global border gap (i x 'I', else j x 'D'): the start is anchored at (0, 0).
 *   The result is (score, a_end = end_i, b_end = end_j); the CIGAR (start -> end, run-length M/I/D, I consumes A)
 *   consumes exactly a_end and b_end.  The empty extension is (0, 0, 0) with the CIGAR "".
 *   A plan reports PairResult{score, status, end_i, end_j}; fin[] holds (H, E, F) at (m, n) as a global plan's does,
 *   and here it IS part of the result: fin[0] = H(m, n) is the end-to-end score -- what msa_nw_align_scored returns --
 *   so a caller decides between clipping and aligning to the end without a second fill.
 *   Out of scope, each MSA_ERR_UNSUPPORTED at plan creation: any band other than -1 (the global plans' |m - n| <= band
 *   does not fit a free end), cells other than MSA_CELLS_DIR / MSA_CELLS_NONE, gap_extend < 0 or gap_open <
 *   gap_extend.  No Z-drop / X-drop termination here: every cell is computed (inside a band:
 *   msa_extend_align_xdrop below).  Such plans always run the stripe kernel
 *   (msa_plan_launch_info mode 0), one pair or a batch, never a split batch; msa_plan_format_info reports end-cell
 *   tracking 1 (compare-select: the tracked values may be negative, which the packed key cannot hold); and the
 *   value-range inequality of msa_plan_create_scored holds unchanged (the same sources, steps and -inf; the tracked
 *   maximum is a copy of a cell).
 * The entries behave as msa_overlap_align / msa_overlap_align_batch and their *32 twins in everything else, in the
 * order documented there: argument, gap, alphabet and range errors decided on the host; admission with the full
 * m x n bytes; chunks of consecutive pairs within a quarter of the budget; a B shared by every pair uploaded once;
 * MSA_ERR_CAPACITY, the batch with the needed size in cigar_off[n_pairs]; n_sym <= 8 under a *32 entry builds exactly
 * the plain entry's plans.  *score, end_ij[2] = {a_end, b_end}, *global_score = H(m, n) (each may be NULL) / score
 * (n_pairs), end_ij (2 n_pairs, required), global_score (n_pairs, or NULL).  cigar(s) == NULL: scores, end cells and
 * global scores from plans without direction bytes. */
int msa_extend_align(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                     const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                     int32_t* global_score, char* cigar, size_t cigar_cap);
int msa_extend_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                           const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                           const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                           int32_t gap_extend, int32_t* score, int64_t* end_ij, int32_t* global_score, char* cigars,
                           size_t cigar_cap, int64_t* cigar_off);
/* ... for alphabets of up to 32 symbols, as msa_fit_align32 is to msa_fit_align (9..32 symbols: MSA_ALG_EXT32 plans) */
int msa_extend_align32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                       const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_ij,
                       int32_t* global_score, char* cigar, size_t cigar_cap);
int msa_extend_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                             const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                             const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                             int32_t gap_extend, int32_t* score, int64_t* end_ij, int32_t* global_score,
                             char* cigars, size_t cigar_cap, int64_t* cigar_off);

/* Banded extension alignment (build extension: MSA_NW_EXTEND_BAND plans; the band of ksw2's "extz", BWA-MEM's and
 * BLAST's gapped extensions): the extension contract of msa_extend_align above with these changes, for a band w >= 0.
 *   Cells: a cell with |i - j| > w is -inf in all three states.  Row 0 and column 0 are the banded global borders:
 *     H(0, j) = -h - g j for 1 <= j <= w, H(i, 0) = F(i, 0) = -h - g i for 1 <= i <= w, -inf beyond.  E, F, H, the
 *     direction byte and every tie rule are exactly a banded MSA_NW_SCORED plan's: the in-band interior bytes of the
 *     two plans on one input are equal.
 *   Result: best = max of H(i, j) over the interior cells with |i - j| <= w; the end cell is the first maximum in
 *     row-major order; best <= 0 is the empty extension (score 0, end cell (0, 0), no walk, empty CIGAR).  The walk is
 *     msa_extend_align's, from the end cell, completed by the global border gap; it never leaves the band, so a stop
 *     at (i, 0) has i <= w and one at (0, j) has j <= w.
 *   The clip rule (what stands for the global plans' |m - n| <= band): a row i > n + w and a column j > m + w hold no
 *     in-band cell, so with m' = min(m, n + w) and n' = min(n, m + w) the problem IS A[0, m') against B[0, n'), and
 *     that pair always has |m' - n'| <= w.  msa_extend_band_clip computes (m', n'); the host entries below clip, a
 *     plan takes clipped sizes and answers |m - n| > band with MSA_ERR_ARG as every banded plan does.
 *   global_score: H(m, n) exists only when nothing was clipped, (m', n') = (m, n); it is then what
 *     msa_nw_align_scored returns under the same band.  Otherwise the entries report MSA_SCORE_NONE.  A plan's
 *     fin[0] is H(m', n'), as for any banded global plan.
 *   One band per call.  band = -1 is not this plan kind's: MSA_NW_EXTEND is untouched and keeps rejecting any band.
 *   Out of scope, each MSA_ERR_UNSUPPORTED at plan creation: band < 0, cells other than MSA_CELLS_DIR /
 *   MSA_CELLS_NONE, a profile (msa_plan_create_profile), gap_extend < 0 or gap_open < gap_extend.  No termination in a plan
 *   (msa_extend_align_xdrop below stops by X-drop, with a kernel of its own); no band,
 *   flow, chunked or split launch: every such plan runs the stripe kernel's exact launch (msa_plan_launch_info mode
 *   0), as every free-end plan does, with end-cell tracking 1.  The value-range inequality of msa_plan_create_scored
 *   holds unchanged (a banded global plan's sources and steps; the tracked maximum is a copy of an in-band cell).
 * The entries are their unbanded twins with `band` after gap_extend, in everything else and in the twins' order of
 * checks: band < 0 is MSA_ERR_ARG, decided with the other arguments; then the gap rule, the alphabet, the device.  Each
 * pair is clipped to (m', n') -- its offsets stay, a prefix is kept -- and a clipped pair's global_score is
 * MSA_SCORE_NONE.  Admission reserves the band's bytes (~(2 band + 64) per row), not the matrix's. */
#define MSA_SCORE_NONE INT32_MIN
/* (m', n') of the clip rule above into *m_eff, *n_eff (either may be NULL).  m, n < 1 or band < 0: MSA_ERR_ARG.  Pure
 * host arithmetic: it needs no device. */
int msa_extend_band_clip(int64_t m, int64_t n, int64_t band, int64_t* m_eff, int64_t* n_eff);
int msa_extend_align_banded(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                            const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                            int64_t* end_ij, int32_t* global_score, char* cigar, size_t cigar_cap);
int msa_extend_align_batch_banded(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                  const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                  const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                  int32_t gap_extend, int64_t band, int32_t* score, int64_t* end_ij,
                                  int32_t* global_score, char* cigars, size_t cigar_cap, int64_t* cigar_off);
/* ... for alphabets of up to 32 symbols (9..32 symbols: MSA_ALG_EXTB32 plans) */
int msa_extend_align_banded32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                              const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                              int64_t* end_ij, int32_t* global_score, char* cigar, size_t cigar_cap);
int msa_extend_align_batch_banded32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                    const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                    const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                    int32_t gap_extend, int64_t band, int32_t* score, int64_t* end_ij,
                                    int32_t* global_score, char* cigars, size_t cigar_cap, int64_t* cigar_off);

/* Banded extension alignment with X-drop termination (build extension; a kernel family of its own, msa_xdrop.hip: one
 * wave per pair sweeps the band anti-diagonal by anti-diagonal and decides after each whether to go on -- not a plan
 * kind: the stripe kernel's schedule is laid out before the launch and computes every cell).  This is the anti-diagonal
 * X-drop of BLAST's gapped extension and LOGAN; ksw2's row-wise Z-drop has a diagonal-offset term, which stays out.
 * Everything is MSA_NW_EXTEND_BAND's on the clipped pair (m', n') = msa_extend_band_clip(m, n, w): the cells, the banded
 * borders, E / F / H, the direction byte and its tie rules, the value-range inequality.  X-drop adds a stopping rule:
 *   d = i + j is a cell's anti-diagonal.  a(d) = the maximum of H over the in-band interior cells on d, -inf when d has
 *   none (band 0, odd d; a(1) = -inf).  best(d) = max(0, a(2), ..., a(d)).
 *   After anti-diagonal d, for d = 2 .. m' + n', the fill stops when   best(d) - max(a(d - 1), a(d)) > xdrop.
 *   D is that d, or m' + n' when the rule never fires; cells with i + j > D do not exist for the result.  (Two
 *   anti-diagonals on purpose: the main diagonal's cells lie on even d only, and a one-anti-diagonal rule would fire at
 *   d = 3 for every xdrop below the gap-open cost.  With w >= 1 every d in [2, m' + n'] holds an in-band interior cell,
 *   with w = 0 every even d does, so the maximum of the two is always finite.)
 *   Result: score and end cell = the first maximum in ROW-MAJOR order over the in-band interior cells with i + j <= D
 *   (not visit order: an equal value on a later anti-diagonal with a smaller row wins); a best <= 0 is the empty
 *   extension exactly as for msa_extend_align_banded; the walk and the border gap are msa_extend_align_banded's (the
 *   walk only meets cells with a smaller i + j: all of them were computed); diagonals = D, per pair; global_score is
 *   MSA_SCORE_NONE when the pair was clipped or D < m' + n'.
 *   xdrop is in raw score units; xdrop < 0 means never stop, and the results are then msa_extend_align_banded's in
 *   every field.
 * Caps: band <= MSA_XDROP_BAND_MAX (per pair three int32 anti-diagonals of 2 band + 4 in LDS, four pairs and 1 KiB of
 * scores per workgroup: 62,656 B at the cap, inside a workgroup's 64 KiB, two workgroups per CU inside its 160 KiB);
 * above it MSA_ERR_UNSUPPORTED.  Lengths have no cap beyond the value-range inequality: one wave fills one pair, so a
 * long pair is simply slow.
 * The entries: the *_banded twins' signatures with `xdrop` after `band` and `diagonals` (n_pairs entries, may be NULL)
 * after `global_score`; the twins' order of checks -- band < 0 is MSA_ERR_ARG with the other arguments; the gap rule
 * and a band above the cap (after the band of the call's longest sequence stood in for a wider one, which holds the
 * same cells) are MSA_ERR_UNSUPPORTED; then the alphabet, and only then the device --; each pair clipped, one symbol
 * map for the call, a shared B uploaded once, chunks within a quarter of the budget, admission with the compact band
 * form's (2 band + 1)(m' + 1) bytes per pair.  Out of scope: ksw2's diagonal-offset term, per-pair bands or xdrop,
 * X-drop for the unbanded extension and for profiles, several waves on one long pair, plan objects. */
#define MSA_XDROP_BAND_MAX 640
int msa_extend_align_xdrop(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                           const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t xdrop,
                           int32_t* score, int64_t* end_ij, int32_t* global_score, int64_t* diagonals, char* cigar,
                           size_t cigar_cap);
int msa_extend_align_batch_xdrop(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                 const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                 const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                 int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* end_ij,
                                 int32_t* global_score, int64_t* diagonals, char* cigars, size_t cigar_cap,
                                 int64_t* cigar_off);
int msa_extend_align_xdrop32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                             const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t xdrop,
                             int32_t* score, int64_t* end_ij, int32_t* global_score, int64_t* diagonals, char* cigar,
                             size_t cigar_cap);
int msa_extend_align_batch_xdrop32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                   const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                   const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                   int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* end_ij,
                                   int32_t* global_score, int64_t* diagonals, char* cigars, size_t cigar_cap,
                                   int64_t* cigar_off);
/* The device-resident form the entries above are built on: asynchronous on `stream`, no allocation, no host sync.
 * dA, dB: device codes (0..31); d_m, d_n, d_a_off, d_b_off: device arrays of n_pairs int64, pair p being
 * dA[a_off[p] .. + m[p]) against dB[b_off[p] .. + n[p]) with CLIPPED sizes, |m - n| <= band (else that pair's status is
 * MSA_ERR_ARG; outside the value-range inequality: MSA_ERR_UNSUPPORTED; such a pair is not filled).  d_sub32: DEVICE
 * table of 1,024 int8 at stride 32, d_sub32[32 a + b] = A's code a against B's code b, or NULL: match / mismatch (in
 * [-128, 127]).  d_dir (may be NULL: no bytes): the direction bytes in a compact band form, cell (i, j) of pair p at
 * d_dir[d_dir_off[p] + i (2 band + 1) + (j - i + band)], rows 0 .. m: (2 band + 1)(m + 1) bytes per pair; the format is
 * msa_plan_traceback_nw's; bytes of cells past D, of borders and outside the band are not written.
 * d_res: 8 int64 per pair, {score, end_i, end_j, D, H(m, n) or MSA_SCORE_NONE when D < m + n, status, in-band interior
 * cells computed (those with i + j <= D), 0}.
 * Host-side errors: a NULL array, n_pairs < 1 or band < 0: MSA_ERR_ARG; gap_extend < 0, gap_open < gap_extend or band >
 * MSA_XDROP_BAND_MAX: MSA_ERR_UNSUPPORTED; then the device.
 * msa_xdrop_extend_walk, after it on the same stream: every pair's walk from its end cell (d_res) over those bytes,
 * one wave per pair; d_ops / d_ops_off / d_info[8 per pair] are msa_plan_traceback_batch's contract (ops end -> start,
 * {n_ops, i + 1, j + 1, status, 0, 0, 0, 0}, (i, j) the border cell where the walk stopped; the caller appends the global
 * border gap; the empty extension is no walk).  Every walk ends within 2 (end_i + end_j) + 4 steps whatever bytes
 * d_dir holds (MSA_ERR_TIMEOUT; a step out of the band or a byte without a predecessor: MSA_ERR_NOMATCH). */
int msa_xdrop_extend_run(const uint8_t* dA, const uint8_t* dB, int64_t n_pairs, const int64_t* d_m,
                         const int64_t* d_n, const int64_t* d_a_off, const int64_t* d_b_off, const int8_t* d_sub32,
                         int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int32_t band,
                         int32_t xdrop, uint8_t* d_dir, const int64_t* d_dir_off, int64_t* d_res, void* stream);
int msa_xdrop_extend_walk(int64_t n_pairs, int32_t band, const uint8_t* d_dir, const int64_t* d_dir_off,
                          const int64_t* d_res, uint8_t* d_ops, const int64_t* d_ops_off, int64_t* d_info,
                          void* stream);
/* msa_xdrop_extend_run with a reading direction per pair: d_step, DEVICE array of n_pairs int8, +1 or -1 (any other
 * value: that pair's status is MSA_ERR_ARG, the other pairs are not affected), or NULL: every pair +1, which is
 * msa_xdrop_extend_run itself.  A pair with step s takes row i's code from dA[a_off + s (i - 1)] and column j's from
 * dB[b_off + s (j - 1)]: with s = -1, a_off and b_off name the bytes nearest the seed, and the pair is the two
 * sequences that end there, read backwards in place -- dA[a_off - m + 1 .. a_off] and dB[b_off - n + 1 .. b_off] must
 * lie inside the buffers.  Everything else is in the pair's own coordinates and as for msa_xdrop_extend_run: the cells,
 * the stopping rule, the tie rules, d_res, the bytes msa_xdrop_extend_walk walks; d_sub32[32 a + b] stays A's code a
 * against B's code b whatever the direction.  Checks and errors: msa_xdrop_extend_run's. */
int msa_xdrop_flank_run(const uint8_t* dA, const uint8_t* dB, int64_t n_pairs, const int64_t* d_m,
                        const int64_t* d_n, const int64_t* d_a_off, const int64_t* d_b_off, const int8_t* d_step,
                        const int8_t* d_sub32, int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend,
                        int32_t band, int32_t xdrop, uint8_t* d_dir, const int64_t* d_dir_off, int64_t* d_res,
                        void* stream);

/* Seed extension (build extension): the alignment through a seed -- A[seed_a .. + seed_len) against
 * B[seed_b .. + seed_len), which the caller found -- extended on both flanks by the X-drop family above, in one call.
 * The left flank is read backwards in place (msa_xdrop_flank_run's step -1): nothing is reversed or copied on the host,
 * and in a batch coinciding ranges (several seeds on one pair, many seeds against one reference) are uploaded once.
 * Contract.  With L = A[:seed_a][::-1] against B[:seed_b][::-1] and R = A[seed_a+seed_len:] against
 * B[seed_b+seed_len:], each flank's result is FIELD FOR FIELD what msa_extend_align_xdrop returns for that pair of byte
 * strings under the same band and xdrop: the band clip, the row-major tie rule in flank coordinates (so for the left
 * flank the end nearest the seed in A, then in B), and the walk's tie order.  Then:
 *   score = flank_score[0] + sum over t of S[A[seed_a+t]][B[seed_b+t]] + flank_score[1]  (the seed may hold mismatches;
 *           seed_len = 0 is a bare anchor);
 *   beg = (seed_a - L.a_end, seed_b - L.b_end);  end = (seed_a + seed_len + R.a_end, seed_b + seed_len + R.b_end);
 *   the CIGAR runs start -> end and consumes exactly end - beg on each side: the left flank's ops IN WALK ORDER (its
 *   walk goes from the far end to the seed, which is left -> right already; its border gap comes after them), then
 *   seed_len x M, then the right flank's ops reversed, run-length encoded once over the whole.  cigar == NULL: no bytes
 *   and no walks.
 *   flank_score (may be NULL) and diagonals (may be NULL): {left, right}.
 * Empty flanks.  A flank with no symbols on either side (seed_a == 0 or seed_b == 0; the seed ending at m or at n) is
 * not launched: its result is the empty extension, score 0, end (0, 0), diagonals 0.  A call whose flanks are all empty
 * makes no device call.
 * Batch: one seed per pair, seed_a / seed_b / seed_len (n_pairs each) relative to the pair; beg_ij, end_ij, flank_score
 * and diagonals hold 2 entries per pair; the other arguments are the batch twins'.
 * Checks, in this order and before any device call.  MSA_ERR_ARG: the alphabet and matrix (as for the twins), a NULL
 * input, a missing score, beg_ij or end_ij, n_pairs < 1, m or n < 1, a range outside the buffers, seed_len < 0,
 * seed_a < 0 or seed_b < 0, seed_a + seed_len > m or seed_b + seed_len > n, band < 0.  MSA_ERR_UNSUPPORTED: band >
 * MSA_XDROP_BAND_MAX (after the band of the call's longest sequence stood in for a wider one), the gap rule, the
 * value-range inequality taken with the whole m + n.  MSA_ERR_ALPHABET: as for the twins.  Then the device: admission
 * with the launched flanks' footprints, ranges of seeds within a quarter of the budget; the two flanks of a seed are
 * neighbouring tasks of one launch.
 * Out of scope: global_score per flank, per-seed bands or xdrop, seeds on the reverse-complement strand (the caller
 * complements), an unbanded seed extension.  (Choosing among several seeds of a pair: msa_chain_seeds, below.) */
int msa_seed_align(const char* A0, size_t m, const char* B0, size_t n, int64_t seed_a, int64_t seed_b,
                   int64_t seed_len, const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                   int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij,
                   int32_t* flank_score, int64_t* diagonals, char* cigar, size_t cigar_cap);
int msa_seed_align_batch(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                         const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                         const int64_t* seed_a, const int64_t* seed_b, const int64_t* seed_len, const char* alphabet,
                         size_t n_sym, const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band,
                         int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij, int32_t* flank_score,
                         int64_t* diagonals, char* cigars, size_t cigar_cap, int64_t* cigar_off);
int msa_seed_align32(const char* A0, size_t m, const char* B0, size_t n, int64_t seed_a, int64_t seed_b,
                     int64_t seed_len, const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                     int32_t gap_extend, int64_t band, int32_t xdrop, int32_t* score, int64_t* beg_ij,
                     int64_t* end_ij, int32_t* flank_score, int64_t* diagonals, char* cigar, size_t cigar_cap);
int msa_seed_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                           const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                           const int64_t* seed_a, const int64_t* seed_b, const int64_t* seed_len, const char* alphabet,
                           size_t n_sym, const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band,
                           int32_t xdrop, int32_t* score, int64_t* beg_ij, int64_t* end_ij, int32_t* flank_score,
                           int64_t* diagonals, char* cigars, size_t cigar_cap, int64_t* cigar_off);

/* Seed chaining (build extension; a kernel family of its own, msa_chain.hip: one wave per problem): the colinear
 * subsets of a pair's anchors with the best scores -- the step between seeding and extension.  All integers, exact.
 * A problem is the list of the N anchors of one pair; anchor t = (a, b, len): A[a .. a + len) seeded against
 * B[b .. b + len), msa_seed_align's coordinates; ae = a + len, be = b + len.  Anchors come in nondecreasing (be, ae)
 * lexicographic order; duplicates are allowed.  One set of parameters per call: match >= 1; gap_open >= gap_extend >= 0,
 * a length difference of L costing gc(L) = (gap_open - gap_extend) + gap_extend L, gc(0) = 0; band >= 0, the largest
 * diagonal skew between neighbours of a chain; max_dist >= 1; lookback in 1 .. MSA_CHAIN_LOOKBACK_MAX.
 *   For j < i, da = ae_i - ae_j and db = be_i - be_j; j may precede i iff i - j <= lookback, da > 0, db > 0,
 *   da <= max_dist, db <= max_dist and |da - db| <= band.
 *     cand(j, i) = f(j) + match min(da, db, len_i) - gc(|da - db|)
 *     f(i)       = max(match len_i, max over admissible j of cand(j, i))
 *     pred(i)    = the LARGEST admissible j with cand(j, i) == f(i) if f(i) > match len_i, else -1
 *   (a candidate that merely equals match len_i is no predecessor, minimap2's `sc > max_f`).  f(i) <= match ae_i, so
 *   int32 holds everything once coordinates are >= 0, len >= 1, ae and be <= 2^26, match 2^26 < 2^30 and
 *   gc(min(band, 2^26)) < 2^30.  band and max_dist above 2^26 act as 2^26.
 * Chains (on the host, O(N log N)): the anchors in order of f descending, ties to the smaller index; from an anchor
 * not yet in a chain follow pred until it is -1 or reaches an anchor u already taken; the chain scores f(end), or
 * f(end) - f(u).  A chain scoring below min_score is dropped, its anchors stay taken.  The kept chains are ranked in
 * that order, rank 0 first.
 * msa_chain_seeds_batch: a, b, len (int64) hold the anchors of all problems back to back, problem p's being
 * off[p] .. off[p + 1] (off: n_problems + 1, off[0] >= 0, ascending, at most 2^26 anchors per problem).  Out, per
 * anchor: f and pred (either may be NULL; pred is an index within the problem), chain_of = the rank of the anchor's
 * chain in its problem, or -1; per problem n_chains; and chain_score (may be NULL): problem p's chains, by rank, at
 * chain_score[off[p] .. off[p] + n_chains[p]).  msa_chain_seeds: one problem of n >= 0 anchors.
 * Errors, in this order.  MSA_ERR_ARG: a NULL a, b, len (with any anchor), off, chain_of or n_chains, n_problems < 1,
 * n < 0, off not as above, a negative coordinate, len < 1, ae or be above 2^26, anchors out of order.
 * MSA_ERR_UNSUPPORTED: a parameter outside its bounds above.  Then the device -- unless no problem holds more than one
 * anchor: such a call is answered on the host (f = match len, pred = -1) and succeeds with or without a GPU.
 * Otherwise: admission against the device budget, ranges of problems within a quarter of it, one launch per range.
 * Out of scope: float / log gap costs as minimap2's, per-problem parameters, a lookback above the cap, minimap2's skip
 * heuristics, reverse-strand anchors (the caller flips them), re-chaining after alignment. */
#define MSA_CHAIN_LOOKBACK_MAX 1024
int msa_chain_seeds(const int64_t* a, const int64_t* b, const int64_t* len, int64_t n, int32_t match,
                    int32_t gap_open, int32_t gap_extend, int64_t band, int64_t max_dist, int32_t lookback,
                    int32_t min_score, int32_t* f, int32_t* pred, int32_t* chain_of, int32_t* n_chains,
                    int32_t* chain_score);
int msa_chain_seeds_batch(const int64_t* a, const int64_t* b, const int64_t* len, int64_t n_problems,
                          const int64_t* off, int32_t match, int32_t gap_open, int32_t gap_extend, int64_t band,
                          int64_t max_dist, int32_t lookback, int32_t min_score, int32_t* f, int32_t* pred,
                          int32_t* chain_of, int32_t* n_chains, int32_t* chain_score);
/* The device-resident form: asynchronous on `stream`, no allocation, no host sync.  d_a, d_b, d_len, d_off: DEVICE
 * arrays as above; d_f, d_pred (per anchor) and d_status (per problem): DEVICE int32.  The kernel checks each problem's
 * anchors and offsets itself: a problem that breaks a rule gets status MSA_ERR_ARG and nothing else is written for it,
 * its neighbours are not affected; N = 0 is status 0 and writes nothing.  Dynamic LDS: four problems x three int32
 * rings of 64 ceil(lookback / 64) + 64 entries per workgroup, 52,224 B at the cap.
 * Host-side errors: a NULL array, n_problems < 1 or > 2^26: MSA_ERR_ARG; a parameter outside its bounds:
 * MSA_ERR_UNSUPPORTED; then the device. */
int msa_chain_run(const int64_t* d_a, const int64_t* d_b, const int64_t* d_len, int64_t n_problems,
                  const int64_t* d_off, int32_t match, int32_t gap_open, int32_t gap_extend, int64_t band,
                  int64_t max_dist, int32_t lookback, int32_t* d_f, int32_t* d_pred, int32_t* d_status, void* stream);

/* The four matrix-scored entries above for alphabets of up to 32 symbols (proteins with B Z X *, IUPAC DNA): the
 * signatures of their 8-symbol twins, 1 <= n_sym <= 32, sub = n_sym x n_sym.  With n_sym <= 8 a call builds exactly
 * the plans its twin builds: the same kernels, the same results.  With 9..32 symbols the codes are 5 bits wide and
 * the plans are msa_plan_create_scored32's (always the stripe kernel; a banded single pair runs its exact masked
 * launch).  n_sym 0 or 33, a duplicate symbol, or a NULL alphabet or sub: MSA_ERR_ARG.  Then, in this order: the other
 * argument errors, the gap rule (MSA_ERR_UNSUPPORTED), the band rule (MSA_ERR_ARG), a symbol of A or B outside the
 * alphabet (MSA_ERR_ALPHABET), and only then the device.  Admission, chunks of pairs, the border gap, the CIGAR
 * format and MSA_ERR_CAPACITY are the twins'.  The 8-symbol entries keep their contract (n_sym == 9: MSA_ERR_ARG). */
int msa_nw_align_scored32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                          const int8_t* sub, int32_t gap_open, int32_t gap_extend, int64_t band, int32_t* score,
                          char* cigar, size_t cigar_cap);
int msa_nw_align_batch_scored32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                int32_t gap_extend, int64_t band, int32_t* score, char* cigars, size_t cigar_cap,
                                int64_t* cigar_off);
int msa_fit_align32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                    const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_j,
                    int64_t* end_j, char* cigar, size_t cigar_cap);
int msa_fit_align_batch32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                          const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                          const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                          int32_t gap_extend, int32_t* score, int64_t* beg_end /* 2 n_pairs: {beg_j, end_j} */,
                          char* cigars, size_t cigar_cap, int64_t* cigar_off);

/* msa_sw_align and msa_sw_align_batch under a substitution matrix (build extension: MSA_SW_SCORED plans): their
 * signatures with `alphabet, n_sym, sub` in place of `match, mismatch`.  alphabet: n_sym distinct bytes, a symbol's
 * code is its index; sub: n_sym x n_sym scores in int8, row-major, the row is A's symbol (it need not be symmetric).
 * The kernels' highest code is their out-of-matrix sentinel, so 1 <= n_sym <= 7 for the plain entries and <= 31 for
 * the *32 entries; up to 7 symbols build exactly the plain entry's plans under either, 8..31 build plans over 5-bit
 * codes (msa_plan_create_scored32).  Every such plan runs the stripe kernel, a single long pair included.
 * n_sym outside that range, a duplicate symbol, or a NULL alphabet or sub: MSA_ERR_ARG.  Then, in this order: the
 * other argument errors, the gap rule (gap_open, gap_extend >= 0, else MSA_ERR_UNSUPPORTED), a symbol of A or B
 * outside the alphabet (MSA_ERR_ALPHABET), and only then the device.  The score, the end cell (first maximum,
 * row-major), the start cell and the CIGAR, score-only calls (cigar and beg NULL), MSA_ERR_CAPACITY (batches: with
 * the needed size in cigar_off[n_pairs]), chunks of pairs, a shared reference and admission against the device
 * budget are msa_sw_align's and msa_sw_align_batch's. */
int msa_sw_align_scored(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                        const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_i,
                        int64_t* end_j, int64_t* beg_i, int64_t* beg_j, char* cigar, size_t cigar_cap);
int msa_sw_align_batch_scored(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                              const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                              const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                              int32_t gap_extend, int32_t* score, int64_t* end_ij, int64_t* beg_ij, char* cigars,
                              size_t cigar_cap, int64_t* cigar_off);
int msa_sw_align_scored32(const char* A0, size_t m, const char* B0, size_t n, const char* alphabet, size_t n_sym,
                          const int8_t* sub, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* end_i,
                          int64_t* end_j, int64_t* beg_i, int64_t* beg_j, char* cigar, size_t cigar_cap);
int msa_sw_align_batch_scored32(const char* A, size_t a_len, const char* B, size_t b_len, int64_t n_pairs,
                                const int64_t* a_off, const int64_t* m, const int64_t* b_off, const int64_t* n,
                                const char* alphabet, size_t n_sym, const int8_t* sub, int32_t gap_open,
                                int32_t gap_extend, int32_t* score, int64_t* end_ij, int64_t* beg_ij, char* cigars,
                                size_t cigar_cap, int64_t* cigar_off);

/* A position-specific score profile against sequences (build extension: msa_plan_create_profile's plans): local
 * (MSA_SW_SCORED's recurrence, end cell and walk), global (MSA_NW_SCORED's, unbanded) or fit (MSA_NW_FIT's: all of
 * the profile in a substring of B).  prof: m x n_sym int8, row-major, prof[n_sym r + c] = the score of profile
 * position r against alphabet[c] -- what a caller's PSSM looks like; the entry pads it to the plans' 32 columns.
 * alphabet: n_sym distinct bytes, the symbols of B, a symbol's code is its index; n_sym is at most 31 for
 * MSA_PROFILE_LOCAL (the highest code is the kernels' sentinel) and at most 32 otherwise.  The batch aligns the ONE
 * profile against n_pairs sequences B[b_off[p] .. b_off[p] + n[p]): every pair uses all m rows.
 * Results, one shape for every mode: score (n_pairs); beg_ij and end_ij, two int64 {i, j} per pair (either may be
 * NULL) -- global: {0, 0} and {m, n}; fit: {0, beg_j} and {m, end_j}, B[beg_j .. end_j) being the substring (beg_j =
 * -1 without a walk); local: the start cell and the end cell as msa_sw_align reports them --; and the CIGAR, start ->
 * end, I consuming a profile row and D a symbol of B.  Score-only calls (cigar NULL; local: and beg_ij NULL),
 * MSA_ERR_CAPACITY (the batch: with the needed size in cigar_off[n_pairs]; cigar_off, n_pairs + 1, is required with
 * cigars), chunks of pairs and a local call's empty result are msa_sw_align_batch_scored32's,
 * msa_nw_align_batch_scored32's and msa_fit_align_batch32's; the profile's 32 bytes per row count against the device
 * budget.
 * Errors, in this order: a mode other than the three, n_sym out of range, a duplicate symbol, or a NULL prof or
 * alphabet: MSA_ERR_ARG; the other argument errors (m, n[p] < 1, a range outside B, n_pairs < 1, a NULL array):
 * MSA_ERR_ARG; the gap rule (local: gap_open, gap_extend >= 0; else gap_open >= gap_extend >= 0):
 * MSA_ERR_UNSUPPORTED; a symbol of B outside the alphabet: MSA_ERR_ALPHABET; and only then the device.
 * Building a PSSM from a multiple alignment -- counts, pseudocounts, log-odds -- is the caller's job. */
enum { MSA_PROFILE_LOCAL = 0, MSA_PROFILE_GLOBAL = 1, MSA_PROFILE_FIT = 2 };
int msa_profile_align(int mode, const int8_t* prof, size_t m, const char* B0, size_t n, const char* alphabet,
                      size_t n_sym, int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij,
                      int64_t* end_ij, char* cigar, size_t cigar_cap);
int msa_profile_align_batch(int mode, const int8_t* prof, size_t m, const char* B, size_t b_len, int64_t n_pairs,
                            const int64_t* b_off, const int64_t* n, const char* alphabet, size_t n_sym,
                            int32_t gap_open, int32_t gap_extend, int32_t* score, int64_t* beg_ij, int64_t* end_ij,
                            char* cigars, size_t cigar_cap, int64_t* cigar_off);

#ifdef __cplusplus
}
#endif

#endif /* MSA_H */

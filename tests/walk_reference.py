"""Synthetic direction planes for the two device traceback walkers (traceback_kernel, traceback_batch_kernel): plain
Python reference walkers, the inverse of Plan.deskew_dir, plane builders, a model of the walkers' group / stripe
geometry, and the case lists of test_gpu_walk_planes.py.

Not a test file.  Numpy and plain Python only; test_walk_reference.py checks all of it on the CPU.

* Reference walkers over a row-major (m+1) x (n+1) byte matrix, written from the contract in msa_traceback.hip's
  header: walk_sw (the SW-affine byte: TB_SW with local=True, TB_NW / TB_FIT with local=False) and walk_gotoh (the
  reference's tables, as numbers or as tags 4 - table).  Every walk ends at i == 0 or j == 0 whatever its state.  A
  Walk holds the ops end -> start, the stop cell, the status, the interior cells the walk stands on in order, and the
  set of states it is in while it stands on each of them (0 / 1 / 2 = H / E / F or T1 / T2 / T3).
* skew_dir: matrix -> skewed stripe layout, the exact inverse of Plan.deskew_dir for one and two rows per lane, from
  plain numbers (Geom and the stripe starts); deskew_rule restates deskew_dir's index rule cell by cell.
* plane_from_ops writes the bytes that make exactly one path (everything else seeded random valid bytes),
  random_plane gives every cell an independent valid byte.  "Valid": every field the walk can read names a
  predecessor inside the matrix -- no plane holds a "no predecessor" code unless a case puts one on its path.
* The geometry model: the step of a cell (t = j - cs + r, or j - cs + (r >> 1) with two rows per lane), group_b0 and
  its clamps, fl_cs, and from a walk's cells the stripes entered, the batch walker's staged groups, a lower bound on
  the single walker's on-demand groups and whether every cell has 0 <= t < 16 pmax.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple

import numpy as np

ERR_CAPACITY, ERR_NOMATCH = -8, -9   # MSA_ERR_CAPACITY, MSA_ERR_NOMATCH (include/msa.h)
TB_RAW, TB_CSL, TBB_CSN, TBB_WPB, GROUP_BLOCKS = 4096, 8192, 512, 4, 16   # the walkers' own constants
GT = 16 * GROUP_BLOCKS   # steps a group covers

Walk = namedtuple("Walk", "ops stop status cells states")
Geom = namedtuple("Geom", "m n pmax rows_per_lane out_off")


# ---- reference walkers -------------------------------------------------------------------------------------------
def walk_sw(byte, end, local: bool) -> Walk:
    """The walk over SW-affine bytes from `end` in state H.  H: low bits 0 stop (local: the alignment starts here;
    global: MSA_ERR_NOMATCH), 1 'M' to the diagonal, 2 -> E, 3 -> F (no op, same cell).  E: 'D', one column left, back
    to H if bit 2.  F: 'I', one row up, back to H if bit 3."""
    i, j = end
    st, status = 0, 0
    ops, cells, states = bytearray(), [], []
    while i > 0 and j > 0:
        if not cells or cells[-1] != (i, j):
            cells.append((i, j))
            states.append(set())
        states[-1].add(st)
        v = int(byte[i, j])
        if st == 0:
            lo = v & 3
            if lo == 0:
                status = 0 if local else ERR_NOMATCH
                break
            if lo == 1:
                ops += b"M"
                i, j = i - 1, j - 1
            else:
                st = lo - 1
        elif st == 1:
            ops += b"D"
            j -= 1
            st = 0 if v & 4 else 1
        else:
            ops += b"I"
            i -= 1
            st = 0 if v & 8 else 2
    return Walk(bytes(ops), (i, j), status, cells, states)


def walk_gotoh(byte, m: int, n: int, end_table: int, tagged: bool) -> Walk:
    """The reference's find_alignment walk from (m, n) in table end_table (1..3).  One op per step, the table the step
    leaves ('M' T1 diagonal, 'D' T2 left, 'I' T3 up); the next table is the cell's field of the table left (bits 0-1 /
    2-3 / 4-5), a table number or, tagged, 4 - it.  A field of 0 (no predecessor) ends the walk after that step with
    MSA_ERR_NOMATCH."""
    i, j, ct, status = m, n, end_table, 0
    ops, cells, states = bytearray(), [], []
    while i > 0 and j > 0:
        cells.append((i, j))
        states.append({ct - 1})
        ops += b"MDI"[ct - 1:ct]
        f = (int(byte[i, j]) >> (2 * (ct - 1))) & 3
        if ct != 2:
            i -= 1
        if ct != 3:
            j -= 1
        if f == 0:
            status = ERR_NOMATCH
            break
        ct = 4 - f if tagged else f
    return Walk(bytes(ops), (i, j), status, cells, states)


def walk_plane(kind: str, byte, end, start_table: int = 1) -> Walk:
    """The reference walk of a plan kind: 'sw' (local), 'nw' (global over SW bytes, any end cell), 'ref', 'tag'."""
    if kind in ("sw", "nw"):
        return walk_sw(byte, end, local=kind == "sw")
    assert tuple(end) == (byte.shape[0] - 1, byte.shape[1] - 1)
    return walk_gotoh(byte, end[0], end[1], start_table, tagged=kind == "tag")


# ---- the layout ----------------------------------------------------------------------------------------------------
def n_stripes(g: Geom) -> int:
    return (g.m + 64 * g.rows_per_lane - 1) // (64 * g.rows_per_lane)


def block_bytes(g: Geom) -> int:
    return n_stripes(g) * g.pmax * 1024 * g.rows_per_lane


def skew_dir(g: Geom, cs, matrix, pad: int, out=None) -> np.ndarray:
    """The flat layout (out_off + the pair's block bytes, or `out`, written in place at out_off) whose deskew_dir is
    `matrix`: stripe s, 16-step block t // 16, row half rho, lane, t % 16 holds cell (64 R s + R lane + rho + 1,
    cs_s + t - lane).  Every layout byte of the block that is no interior matrix cell is `pad`."""
    R, S, T = g.rows_per_lane, n_stripes(g), 16 * g.pmax
    if out is None:
        out = np.full(g.out_off + block_bytes(g), pad, dtype=np.uint8)
    blk = out[g.out_off:g.out_off + block_bytes(g)].reshape(S, g.pmax, R, 64, 16)
    blk[...] = pad
    t = np.arange(T)
    lane = np.arange(64)
    for s in range(S):
        j = int(cs[s]) + t[None, :] - lane[:, None]
        okj = (j >= 1) & (j <= g.n)
        jj = np.where(okj, j, 0)
        for rho in range(R):
            i = 64 * R * s + R * lane + rho + 1
            ok = okj & (i[:, None] <= g.m)
            ii = np.broadcast_to(np.minimum(i, g.m)[:, None], j.shape)
            vals = np.where(ok, matrix[ii, jj], pad).astype(np.uint8)   # [lane][t]
            blk[s, :, rho] = vals.reshape(64, g.pmax, 16).transpose(1, 0, 2)
    return out


def layout_index(g: Geom, cs, i: int, j: int) -> int:
    """deskew_dir's index rule for one cell, in plain arithmetic: the flat index of cell (i, j)."""
    R = g.rows_per_lane
    s, r = (i - 1) // (64 * R), (i - 1) % (64 * R)
    lane, rho = r // R, r % R
    t = j - int(cs[s]) + lane
    assert 0 <= t < 16 * g.pmax, (i, j, t)
    return g.out_off + (((s * g.pmax + t // 16) * R + rho) * 64 + lane) * 16 + t % 16


def layout_indices(g: Geom, cs, cells) -> np.ndarray:
    """layout_index of many cells at once."""
    R = g.rows_per_lane
    ij = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    s, r = (ij[:, 0] - 1) // (64 * R), (ij[:, 0] - 1) % (64 * R)
    lane, rho = r // R, r % R
    t = ij[:, 1] - np.asarray(cs, dtype=np.int64)[s] + lane
    assert ((t >= 0) & (t < 16 * g.pmax)).all()
    return g.out_off + (((s * g.pmax + t // 16) * R + rho) * 64 + lane) * 16 + t % 16


def deskew_rule(g: Geom, cs, flat) -> np.ndarray:
    """deskew_dir restated cell by cell through layout_index (cells the layout does not hold stay 0)."""
    out = np.zeros((g.m + 1, g.n + 1), dtype=np.uint8)
    R = g.rows_per_lane
    for i in range(1, g.m + 1):
        s, lane = (i - 1) // (64 * R), ((i - 1) % (64 * R)) // R
        for j in range(1, g.n + 1):
            if 0 <= j - int(cs[s]) + lane < 16 * g.pmax:
                out[i, j] = flat[layout_index(g, cs, i, j)]
    return out


# ---- the geometry of the fills (restated: plan.stripe_geom, msa_flow.hip's fl_cs / fl_P) -------------------------
def fl_cs(k: int) -> int:
    return -((16 - (k & 15)) & 15)


def stripe_cs_P(k: int, m: int, n: int, band: int = -1):
    """(cs, 16-step blocks) of stripe k of a one-row-per-lane plan (stripe_geom with 16 steps per phase)."""
    i0 = 64 * k + 1
    rlast = min(63, m - 64 * k - 1)
    clo = 1 if band < 0 else max(1, i0 - band)
    cs = clo - ((clo - 1 - k) % 16 + 1)
    jhi = n if band < 0 else min(n, i0 + rlast + band)
    return cs, (jhi - cs + rlast) // 16 + 1


def model_geom(m: int, n: int, rows_per_lane: int = 1, band: int = -1, out_off: int = 0):
    """(Geom, stripe starts) a plan of this shape has: the stripe kernel's rule (any band) or, two rows per lane, the
    flow kernels' (fl_cs, fl_P).  The GPU tests assert that the plans' own numbers equal these."""
    if rows_per_lane == 2:
        S = (m + 127) // 128
        cs = [fl_cs(k) for k in range(S)]
        # (the plan lays a flow pair out for the larger of the flow kernels' block count, fl_P, and the stripe rule's)
        P = [(n - cs[k] + min((m - 128 * k - 1) // 2, 63)) // 16 + 1 for k in range(S)]
        P += [stripe_cs_P(k, m, n)[1] for k in range((m + 63) // 64)]
    else:
        S = (m + 63) // 64
        cs, P = zip(*(stripe_cs_P(k, m, n, band) for k in range(S)))
    return Geom(m, n, max(P), rows_per_lane, out_off), list(cs)


def group_b0(t: int, pmax: int) -> int:
    """The first block of the 16-block group that ends a little right of step t, clamped to the stripe's blocks."""
    b0 = ((t + 16) >> 4) - (GROUP_BLOCKS - 1)
    b0 = min(b0, pmax - GROUP_BLOCKS)
    return max(b0, 0)


def locate(g: Geom, cs, i: int, j: int):
    """(stripe, row in the stripe, step) of an interior cell."""
    SR = 64 * g.rows_per_lane
    s, r = (i - 1) // SR, (i - 1) % SR
    return s, r, j - int(cs[s]) + (r >> 1 if g.rows_per_lane == 2 else r)


def steps_in_range(g: Geom, cs, cells) -> bool:
    return all(0 <= locate(g, cs, i, j)[2] < 16 * g.pmax for i, j in cells)


def inside(g: Geom, cells, band: int = -1) -> bool:
    return all(1 <= i <= g.m and 1 <= j <= g.n and (band < 0 or abs(i - j) <= band) for i, j in cells)


def inside_mask(m: int, n: int, band: int) -> np.ndarray:
    """The interior cells of the (m+1) x (n+1) matrix, inside the band if there is one."""
    i, j = np.arange(m + 1)[:, None], np.arange(n + 1)[None, :]
    return (i >= 1) & (j >= 1) & ((band < 0) | (np.abs(i - j) <= band))


def stripes_entered(g: Geom, cells) -> int:
    SR = 64 * g.rows_per_lane
    s = [(i - 1) // SR for i, _ in cells]
    return sum(1 for k in range(len(s)) if k == 0 or s[k] != s[k - 1])


def _covered(b0, t):
    return b0 is not None and 16 * b0 <= t < 16 * b0 + GT


def batch_groups(g: Geom, cs, cells, trace=None) -> int:
    """Groups the batch walker stages: one at the first cell, then one at every cell the current group (its stripe,
    its 256 steps) does not cover.  trace, if a list, receives (cell index, stripe, b0, left) per staging, left =
    the walk left its group on the left inside one stripe."""
    gs, b0, n = -1, None, 0
    for k, (i, j) in enumerate(cells):
        s, _, t = locate(g, cs, i, j)
        if gs != s or not _covered(b0, t):
            left = gs == s
            gs, b0, n = s, group_b0(t, g.pmax), n + 1
            if trace is not None:
                trace.append((k, s, b0, left))
    return n


def left_exits(g: Geom, cs, cells) -> int:
    tr = []
    batch_groups(g, cs, cells, tr)
    return sum(1 for x in tr if x[3])


def demand_lower_bound(g: Geom, cs, cells) -> int:
    """A lower bound on the groups the single walker's loaders stage on request.  The first stripe's group is always
    requested.  A later stripe sd was prefetched, if at all, when the walk entered stripe sd + d (d = 1..3) at column
    hint `col` = j - r: the group of step col - 64 d + 126 - cs (two rows per lane: col - 128 d + 190 - cs), or it is
    requested before any prefetch lands.  Which of these happened depends on timing, so the bound takes, per stripe,
    the fewest requests over all of them (a hint read while the walker rewrites it pairs stripe sd + d with the next
    entry's column: those count as candidates too): the entry if the group does not cover it -- always so more than 31
    steps right of the prediction --, then every exit on the left."""
    R, SR = g.rows_per_lane, 64 * g.rows_per_lane
    per, order, col = {}, [], {}
    for i, j in cells:
        s, r, t = locate(g, cs, i, j)
        if s not in per:
            per[s] = []
            order.append(s)
            col[s] = j - r
        per[s].append(t)

    def requests(b0, ts):
        nreq = 0
        for t in ts:
            if not _covered(b0, t):
                b0, nreq = group_b0(t, g.pmax), nreq + 1
        return nreq

    total = 0
    for s in order:
        cand = [None]
        for d in (1, 2, 3):
            for e in (s + d, s + d - 1):
                if s + d in col and e in col:
                    pred = col[e] - (128 * d - 190 if R == 2 else 64 * d - 126) - int(cs[s])
                    cand.append(group_b0(pred, g.pmax))
        if s == order[0]:
            cand = [None]
        total += min(requests(b0, per[s]) for b0 in cand)
    return total


# ---- plane builders ------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def random_plane(kind: str, m: int, n: int, share: float, seed) -> np.ndarray:
    """Every interior cell an independent valid byte (row and column 0 are 0).  SW kinds: the low bits 1 with
    probability `share` (in 256ths), else 2 or 3; bits 2 and 3 random.  Gotoh kinds: T1's field names T1 with
    probability `share`, else T2 or T3; T2's and T3's fields are drawn from the three tables.  The bits no walk reads
    are random too."""
    rng = _rng("plane", kind, m, n, share, seed)
    shp = (m + 1, n + 1)
    r1 = rng.integers(0, 256, shp, dtype=np.uint8)
    r2 = rng.integers(0, 256, shp, dtype=np.uint8)
    pick = np.where(r1 < int(round(share * 256)), 1, 2 + (r2 >> 7)).astype(np.uint8)
    if kind in ("sw", "nw"):
        p = (r2 << 2) | pick   # bits 2-3 and the unread bits 4-7 from r2
    else:
        f2, f3 = r2 % 3 + 1, (r2 // 3) % 3 + 1   # table numbers
        if kind == "tag":
            pick, f2, f3 = 4 - pick, 4 - f2, 4 - f3
        p = pick | (f2 << 2) | (f3 << 4) | ((r1 & 3) << 6)
    p = p.astype(np.uint8)
    p[0, :] = 0
    p[:, 0] = 0
    return p


def expand(segs):
    """(ops, reopen) of a path given as [(letter, count)] end -> start: two consecutive segments of one gap letter
    are two gaps, the first closing on the cell the second opens from (reopen = the op indices that close so)."""
    ops, reopen = bytearray(), set()
    for k, (op, c) in enumerate(segs):
        assert c >= 0 and op in "MDI"
        if c == 0:
            continue
        ops += op.encode() * c
        nxt = next((o for o, cc in segs[k + 1:] if cc > 0), None)
        if op != "M" and nxt == op:
            reopen.add(len(ops) - 1)
    return bytes(ops), reopen


def apply_path(kind: str, p, ops: bytes, end, reopen=(), local_stop=False, nomatch=False) -> list:
    """Overwrite, in place, the fields of plane p that the walk from `end` (Gotoh kinds: in the table of ops[0]) reads
    along the path `ops`, so that it makes exactly those ops; returns the cells written.  The path must end on the
    border, or, with local_stop (SW) / nomatch (a global walk over SW bytes), in state H on an interior cell that gets
    low bits 0.  A gap op closes (returns to H) when the next op differs, when its index is in `reopen`, or before such
    a stop; the last gap op of a path to the border stays open: the walk reaches the border in state E or F."""
    i, j = end
    cells = []
    if kind in ("sw", "nw"):
        st, k = 0, 0
        while k < len(ops):
            assert 1 <= i <= p.shape[0] - 1 and 1 <= j <= p.shape[1] - 1, (i, j, k)
            op = ops[k:k + 1]
            cells.append((i, j))
            if st == 0:
                if op == b"M":
                    p[i, j] = (int(p[i, j]) & 0xFC) | 1
                    i, j, k = i - 1, j - 1, k + 1
                else:
                    st = 1 if op == b"D" else 2
                    p[i, j] = (int(p[i, j]) & 0xFC) | (st + 1)
                continue
            assert op == (b"D" if st == 1 else b"I"), (k, op, st)
            last = k + 1 == len(ops)
            close = k in reopen or (not last and ops[k + 1:k + 2] != op) or (last and (local_stop or nomatch))
            bit = 4 if st == 1 else 8
            p[i, j] = (int(p[i, j]) & (0xFF ^ bit)) | (bit if close else 0)
            if st == 1:
                j -= 1
            else:
                i -= 1
            st, k = (0 if close else st), k + 1
        if local_stop or nomatch:
            assert st == 0 and 1 <= i <= p.shape[0] - 1 and 1 <= j <= p.shape[1] - 1, (i, j, st)
            p[i, j] = int(p[i, j]) & 0xFC
            cells.append((i, j))
        else:
            assert i == 0 or j == 0, (i, j)
    else:
        assert not (local_stop or nomatch)
        for k in range(len(ops)):
            assert 1 <= i <= p.shape[0] - 1 and 1 <= j <= p.shape[1] - 1, (i, j, k)
            ct = b"MDI".index(ops[k:k + 1]) + 1
            if k + 1 < len(ops):
                nt = b"MDI".index(ops[k + 1:k + 2]) + 1
                sh = 2 * (ct - 1)
                p[i, j] = (int(p[i, j]) & (0xFF ^ (3 << sh))) | ((4 - nt if kind == "tag" else nt) << sh)
                cells.append((i, j))
            if ct != 2:
                i -= 1
            if ct != 3:
                j -= 1
        assert i == 0 or j == 0, (i, j)
    return cells


def plane_from_ops(kind: str, m: int, n: int, ops: bytes, end, reopen=(), local_stop=False, nomatch=False, seed=0,
                   share=0.5) -> np.ndarray:
    """The plane whose walk from `end` makes exactly `ops` (apply_path) over seeded random valid bytes everywhere
    else: a walker that reads a neighbouring cell goes astray."""
    p = random_plane(kind, m, n, share, ("path", seed))
    apply_path(kind, p, ops, end, reopen, local_stop, nomatch)
    return p


def consumed(ops: bytes):
    """(rows, columns) the ops consume."""
    return len(ops) - ops.count(b"D"), len(ops) - ops.count(b"I")


def to_border(segs, end):
    """segs + the diagonal from where they end to the matrix border."""
    di, dj = consumed(expand(segs)[0])
    i, j = end[0] - di, end[1] - dj
    assert i >= 0 and j >= 0, (i, j)
    return list(segs) + [("M", min(i, j))]


# ---- the cases -----------------------------------------------------------------------------------------------------
PADS = (0x01, 0x02, 0x0F)
SHARES = (0.2, 0.6, 0.95)
SEEDS = 20
# (a) one row per lane, each next to the boundary it sits on:
SHAPES_A = [
    (1, 1),       # one cell
    (7, 9),       # less than a window
    (63, 70),     # one short of a stripe
    (64, 64),     # exactly one stripe
    (65, 300),    # the second stripe has one row; pmax >= 16
    (130, 150),   # three stripes of fewer than 16 blocks: the glds16 path, the last block loaded again
    (130, 190),   # 17 blocks, one more than a group: b0 is 0 or 1
    (200, 260),   # pmax >= 16 with b0 clamped at 0 and at pmax - 16
    (600, 700),   # more stripes than LDS slots: every slot is reused
]
# the batch of (a): those and two with more rows than columns; no multiple of TBB_WPB, so the last workgroup has an
# idle wave
BATCH_SHAPES = SHAPES_A + [(70, 63), (300, 65)]
# (a) two rows per lane: the shapes of flow_dir_reference.SHAPES with m = 127, 128, 129 (one stripe | two), 513 (a
# stripe of one row) and 2,200 (18 stripes: fl_cs wraps at stripe 16)
FLOW_MS = (127, 128, 129, 513, 2200)


def flow_shapes():
    import flow_dir_reference as FR

    return [s for s in FR.SHAPES if s[0] in FLOW_MS]


# (b) constructed paths
SHAPES_B = [(700, 900), (2200, 2300)]
HGAPS = (239, 240, 241, 256, 257, 700)   # a group covers 256 steps and ends 16..31 right of the entry
VGAPS = (20, 64, 65, 200, 300)           # 0..4 stripes crossed straight up: the prefetch predicted a diagonal
STAIRS = (50, 500)
RUNS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)   # a run probe reads 64 (two rows per lane: 128) cells
BANDS = (16, 64)
BAND_M = 700


def _runs_segs(L: int):
    """16 diagonal runs of L between single gap ops -- one 'D', or 'D' then 'I' where that makes the period odd --, so
    that the runs start at all 16 residues of their op index."""
    gap = [("D", 1)] if L % 2 == 0 else [("D", 1), ("I", 1)]
    return [x for _ in range(16) for x in [("M", L)] + gap]


def run_starts(ops: bytes, L: int):
    """The op indices at which the maximal 'M' runs of exactly L begin."""
    out, k = [], 0
    while k < len(ops):
        if ops[k:k + 1] == b"M":
            e = k
            while e < len(ops) and ops[e:e + 1] == b"M":
                e += 1
            if e - k == L:
                out.append(k)
            k = e
        else:
            k += 1
    return out


def path_cases(m: int, n: int, rows_per_lane: int = 1, local=False):
    """{name: dict(segs, local_stop)} of the constructed paths of an unbanded m x n matrix walked from (m, n), in the
    layout with that many rows per lane.  Global paths run to the border; with local=True (SW) the paths named local_*
    end in a local start."""
    end = (m, n)
    ei, ej = end
    SR = 64 * rows_per_lane
    r0 = (ei - 1) % SR
    g, cs = model_geom(m, n, rows_per_lane)
    # `edge`: from (m, n) a few columns left, then diagonally into the bottom row of the stripe above, entered at a
    # step t = 15 mod 16: the group staged there begins at t - 239, so a gap of 239 ends on the group's first step and
    # one of 240 leaves the group on the left
    k16 = (locate(g, cs, ei - r0 - 1, ej - r0 - 1)[2] - 15) % 16
    edge = [("D", k16), ("M", r0 + 1)]
    c = {}

    def add(name, segs, stop=False):
        c[name] = dict(segs=list(segs) if stop else to_border(segs, end), local_stop=stop)

    # a horizontal gap inside one stripe row, opened on the cell where a diagonal enters the stripe above
    for L in HGAPS:
        add(f"hgap{L}", edge + [("D", L)])
    # ... and one that closes on the group's first step, where a vertical gap opens
    add("group_first_step_F", edge + [("D", 239), ("I", 3)])
    # a vertical gap: the next stripes are entered straight above, not where a diagonal would
    for L in VGAPS:
        add(f"vgap{L}", [("M", 10), ("I", L)])
    # gaps that close and reopen on the next cell, and E -> H -> F corners
    add("reopen", [("M", 5), ("D", 3), ("D", 1), ("D", 2), ("I", 2), ("I", 2), ("M", 3), ("I", 1), ("D", 1),
                   ("I", 70), ("I", 1), ("D", 300), ("D", 1), ("M", 2)])
    for k in STAIRS:
        add(f"stair{k}", [("M", 3)] + [("D", 1), ("I", 1)] * k)
    # the four edges: up column n and along row 1 to the corner; along row m and up column 1
    add("col_n_row_1", [("I", ei - 1), ("D", ej - 1)])
    add("row_m_col_1", [("D", ej - 1), ("I", ei - 1)])
    # the border reached in state E and in state F (every other global path reaches it in H)
    add("border_E", [("M", 7), ("I", ei - 7 - 3), ("D", ej - 7)])
    add("border_F", [("M", 7), ("D", ej - 7 - 5), ("I", ei - 7)])
    # along a stripe's top row across group edges in state E, then up across stripe tops in state F
    add("top_row_E", [("M", r0), ("D", 600), ("I", 130), ("D", 40)])
    # diagonal runs between single gaps at every byte alignment of the ops
    for L in RUNS:
        if 16 * (L + 2) < min(ei, ej):
            add(f"runs{L}", _runs_segs(L))
    if local:
        # a local start after 0..7 alternating single gaps: every step position of a window
        for k in range(8):
            add(f"local_pos{k}", ([("D", 1), ("I", 1)] * 4)[:k], stop=True)
        # a local start on a stripe's top row, right after a stripe entry, and left of a group
        add("local_top_row", [("M", r0)], stop=True)
        add("local_stripe_entry", [("M", r0 + 1)], stop=True)
        for L in (238, 239, 240, 256, 257):
            add(f"local_after_hgap{L}", edge + [("D", L)], stop=True)
        add("local_after_vgap", [("M", 10), ("I", 200)], stop=True)
        add("local_row_1", [("I", ei - 1), ("D", 5)], stop=True)
        add("local_col_1", [("D", ej - 1), ("I", 5)], stop=True)
    return c


def band_cases(w: int, m: int = BAND_M):
    """Paths of a banded m x m plan from (m, m): on the lower band edge i - j = +w, on the upper one i - j = -w, and
    one that switches between the two."""
    end = (m, m)
    return {
        "edge_plus": to_border([("D", w)], end),
        "edge_minus": to_border([("I", w)], end),
        "switch": to_border([("D", w), ("M", 150), ("I", 2 * w), ("M", 150), ("D", 2 * w), ("M", 100), ("I", 2 * w)],
                            end),
    }


# (c) / (d): the long vertical-dominant path
RING_SHAPE = (72000, 320)          # >= 71,680 ops at <= 7 ops per ring word: >= 10,240 words, 2.5 laps of the ring
RING_MIN_OPS = 71680
STARTS_SHAPE = (64 * TB_CSL + 65, 96)   # 8,194 stripes: the last two start columns come from memory
CAP = 1000


@functools.lru_cache(maxsize=None)
def tall_ops(m: int, n: int) -> bytes:
    """From (m, n) to row 0: 'I' runs of m // n rows with one 'M' or one 'D' (in turn) between them -- no two
    consecutive 'M', at least m ops."""
    q = m // n
    ops, i, j, k = bytearray(), m, n, 0
    while i > 0 and j > 0:
        c = min(q, i)
        ops += b"I" * c
        i -= c
        if i > 0 and j > 1:
            if k % 2 == 0:
                ops += b"M"
                i -= 1
            else:
                ops += b"D"
            j -= 1
            k += 1
    assert i == 0 and j >= 1
    return bytes(ops)


# (e) the real noisy pair
NOISY = dict(m=6000, sub=0.08, indel=0.06, seed=606, sw=(2, -3, 5, 2), gh=(1, 0), min_gap_runs=300)


@functools.lru_cache(maxsize=None)
def noisy_pair():
    import nw_reference as NW

    A, B = NW.similar(np.random.default_rng(NOISY["seed"]), NOISY["m"], sub=NOISY["sub"], indel=NOISY["indel"])
    return (A, B) if len(A) <= len(B) else (B, A)   # (rows <= columns: the oracle's Subproblem swaps any other pair)


def gap_runs(ops: bytes) -> int:
    return sum(1 for k in range(len(ops)) if ops[k:k + 1] != b"M" and (k == 0 or ops[k - 1:k] != ops[k:k + 1]))

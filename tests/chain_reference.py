"""Seed chaining in plain Python: the yardstick of the chain tests.

Not a test file.  The contract is include/msa.h's at msa_chain_seeds.  Anchor t = (a, b, len): A[a : a + len] seeded
against B[b : b + len]; ae = a + len, be = b + len; the anchors of a problem come in nondecreasing (be, ae) order.  For
j < i, da = ae_i - ae_j and db = be_i - be_j; j may precede i iff i - j <= lookback, 0 < da <= max_dist,
0 < db <= max_dist and |da - db| <= band.  Then

    cand(j, i) = f(j) + match min(da, db, len_i) - gc(|da - db|)       gc(L) = (gap_open - gap_extend) + gap_extend L,
    f(i)       = max(match len_i, max over admissible j of cand(j, i))  gc(0) = 0
    pred(i)    = the LARGEST admissible j with cand(j, i) == f(i) if f(i) > match len_i, else -1

written as the O(N lookback) double loop it is, with no early stop.  Chains: the anchors by f descending, ties to the
smaller index; from one not yet taken follow pred until -1 or a taken anchor u; the score is f(end), or f(end) - f(u);
below min_score the chain is dropped and its anchors stay taken; the kept ones are ranked in that order.

plan() is the composition api.chain_align is defined as: the anchors of a chain trimmed to their last
k = min(da, db, len_i) columns, the regions between them, and the two outer flanks.
"""
from __future__ import annotations

import numpy as np

LIMIT = 1 << 26


def gc(L: int, gap_open: int, gap_extend: int) -> int:
    return 0 if L == 0 else (gap_open - gap_extend) + gap_extend * L


def sort_order(a, b, ln):
    """The caller's indices in (be, ae, index) order."""
    a, b, ln = (np.asarray(x, dtype=np.int64) for x in (a, b, ln))
    return sorted(range(len(a)), key=lambda t: (int(b[t] + ln[t]), int(a[t] + ln[t]), t))


def is_sorted(a, b, ln) -> bool:
    keys = [(int(y + l), int(x + l)) for x, y, l in zip(a, b, ln)]
    return all(k0 <= k1 for k0, k1 in zip(keys, keys[1:]))


def recurrence(a, b, ln, band, match=1, gap_open=3, gap_extend=1, max_dist=5000, lookback=64):
    """(f, pred) of one problem whose anchors are in order: two lists of int."""
    assert is_sorted(a, b, ln)
    band, max_dist = min(band, LIMIT), min(max_dist, LIMIT)
    ae = [int(x + l) for x, l in zip(a, ln)]
    be = [int(y + l) for y, l in zip(b, ln)]
    f, pred = [], []
    for i in range(len(ae)):
        best, who = match * int(ln[i]), -1
        for j in range(max(0, i - lookback), i):   # ascending j and >=: the largest j of the maximum stays
            da, db = ae[i] - ae[j], be[i] - be[j]
            if not (0 < da <= max_dist and 0 < db <= max_dist and abs(da - db) <= band):
                continue
            cand = f[j] + match * min(da, db, int(ln[i])) - gc(abs(da - db), gap_open, gap_extend)
            if cand > best or (cand == best and who >= 0):
                best, who = cand, j
        f.append(best)
        pred.append(who)
    return f, pred


def extract(f, pred, min_score=0):
    """(chain_of per anchor, the kept chains' scores by rank)."""
    n = len(f)
    chain_of, taken, scores = [-1] * n, [False] * n, []
    for end in sorted(range(n), key=lambda t: (-f[t], t)):
        if taken[end]:
            continue
        members, u = [], end
        while u >= 0 and not taken[u]:
            taken[u] = True
            members.append(u)
            u = pred[u]
        score = f[end] - (f[u] if u >= 0 else 0)
        if score < min_score:
            continue
        for t in members:
            chain_of[t] = len(scores)
        scores.append(score)
    return chain_of, scores


def chain_reference(a, b, ln, band, match=1, gap_open=3, gap_extend=1, max_dist=5000, lookback=64, min_score=0):
    """dict(f, pred, chain_of, n_chains, chain_score) of one problem in order."""
    f, pred = recurrence(a, b, ln, band, match, gap_open, gap_extend, max_dist, lookback)
    chain_of, scores = extract(f, pred, min_score)
    return dict(f=f, pred=pred, chain_of=chain_of, n_chains=len(scores), chain_score=scores)


def chains(a, b, ln, band, **kw):
    """api.chain_seeds' list for anchors in ANY order: dict(score, anchors (the caller's indices, chain order), a_beg,
    b_beg, a_end, b_end), rank 0 first."""
    order = sort_order(a, b, ln)
    sa, sb, sl = ([int(x[t]) for t in order] for x in (a, b, ln))
    r = chain_reference(sa, sb, sl, band, **kw)
    out = []
    for rank in range(r["n_chains"]):
        pos = [k for k, c in enumerate(r["chain_of"]) if c == rank]
        first, last = pos[0], pos[-1]
        out.append(dict(score=r["chain_score"][rank], anchors=[order[k] for k in pos], a_beg=sa[first], b_beg=sb[first],
                        a_end=sa[last] + sl[last], b_end=sb[last] + sl[last]))
    return out


def plan(a, b, ln, anchors):
    """The parts of the alignment through the chain `anchors` (indices into a, b, ln, chain order) -> dict(left =
    (a_beg, b_beg): the left flank is A[:a_beg][::-1] against B[:b_beg][::-1]; parts = in order ("seed", a0, a1, b0, b1)
    -- A[a0:a1] against B[b0:b1] column by column, a1 - a0 == b1 - b0 >= 1 -- and ("gap", a0, a1, b0, b1) -- the region
    between two anchors, at least one side non-empty; right = (a_end, b_end): the right flank is A[a_end:] against
    B[b_end:])."""
    t0 = anchors[0]
    pae, pbe = int(a[t0] + ln[t0]), int(b[t0] + ln[t0])
    parts = [("seed", int(a[t0]), pae, int(b[t0]), pbe)]
    for t in anchors[1:]:
        ae, be = int(a[t] + ln[t]), int(b[t] + ln[t])
        da, db = ae - pae, be - pbe
        k = min(da, db, int(ln[t]))
        assert k >= 1
        if da > k or db > k:
            assert k == int(ln[t]) or da == k or db == k   # after trimming at most one side of the gap is non-empty
            parts.append(("gap", pae, ae - k, pbe, be - k))
        parts.append(("seed", ae - k, ae, be - k, be))
        pae, pbe = ae, be
    return dict(left=(int(a[t0]), int(b[t0])), parts=parts, right=(pae, pbe))

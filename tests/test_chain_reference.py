"""The chaining yardstick (tests/chain_reference.py) on cases worked by hand.  match 1, gap_open 3, gap_extend 1 unless a
case says otherwise: gc(L) = 2 + L.  Nothing here needs the library or a GPU."""
import chain_reference as CR


def _cols(anchors):
    return tuple([t[k] for t in anchors] for k in range(3))


def test_two_colinear_anchors():
    # ae = be = 10 and 30: da = db = 20, min(20, 20, 10) = 10, no skew: 10 + 10
    r = CR.chain_reference(*_cols([(0, 0, 10), (20, 20, 10)]), band=0)
    assert (r["f"], r["pred"]) == ([10, 20], [-1, 0])
    assert (r["chain_of"], r["n_chains"], r["chain_score"]) == ([0, 0], 1, [20])


def test_skew_exceeds_the_band():
    # da = 20, db = 30: skew 10
    cols = _cols([(0, 0, 10), (20, 30, 10)])
    r = CR.chain_reference(*cols, band=9)
    assert (r["f"], r["pred"]) == ([10, 10], [-1, -1])
    assert (r["chain_of"], r["n_chains"], r["chain_score"]) == ([0, 1], 2, [10, 10])   # equal f: the smaller index first
    # inside the band the gap still has to pay: 10 + 10 - gc(10) = 8 < 10 ...
    assert CR.chain_reference(*cols, band=10)["pred"] == [-1, -1]
    # ... and with gc(10) = 1 it does: 19
    r = CR.chain_reference(*cols, band=10, gap_open=1, gap_extend=0)
    assert (r["f"], r["pred"], r["chain_score"]) == ([10, 19], [-1, 0], [19])
    # max_dist bounds both sides: db = 30
    assert CR.chain_reference(*cols, band=10, gap_open=1, gap_extend=0, max_dist=29)["pred"] == [-1, -1]
    assert CR.chain_reference(*cols, band=10, gap_open=1, gap_extend=0, max_dist=30)["pred"] == [-1, 0]


def test_overlapping_kmers_at_stride_1():
    # da = db = 1 < len: each adds one column
    a, b, ln = _cols([(0, 0, 5), (1, 1, 5), (2, 2, 5), (3, 3, 5)])
    r = CR.chain_reference(a, b, ln, band=0)
    assert (r["f"], r["pred"], r["chain_score"]) == ([5, 6, 7, 8], [-1, 0, 1, 2], [8])
    # lookback 1 is enough here; so is max_dist 1
    assert CR.chain_reference(a, b, ln, band=0, lookback=1, max_dist=1)["f"] == [5, 6, 7, 8]
    p = CR.plan(a, b, ln, [0, 1, 2, 3])
    assert p == dict(left=(0, 0), parts=[("seed", 0, 5, 0, 5), ("seed", 5, 6, 5, 6), ("seed", 6, 7, 6, 7),
                                         ("seed", 7, 8, 7, 8)], right=(8, 8))


def test_tie_between_two_predecessors():
    # anchors 0 and 1 end at (5, 5) and (5, 6): 1 cannot follow 0 (da = 0).  Anchor 2 ends at (24, 24); with free gaps
    # both give 5 + 4 = 9: the larger j wins
    cols = _cols([(0, 0, 5), (0, 1, 5), (20, 20, 4)])
    r = CR.chain_reference(*cols, band=1, gap_open=0, gap_extend=0)
    assert (r["f"], r["pred"]) == ([5, 5, 9], [-1, -1, 1])
    assert (r["chain_of"], r["chain_score"]) == ([1, 0, 0], [9, 5])
    # with gc(1) = 3 anchor 1 gives 6 and anchor 0 wins
    assert CR.chain_reference(*cols, band=1)["pred"] == [-1, -1, 0]
    # lookback 1 sees anchor 1 alone
    assert CR.chain_reference(*cols, band=0, lookback=1)["pred"] == [-1, -1, -1]


def test_candidate_equal_to_the_anchor_alone():
    # da = 13, db = 16: 5 + min(13, 16, 8) - gc(3) = 8 = match * len: no predecessor
    r = CR.chain_reference(*_cols([(0, 0, 5), (10, 13, 8)]), band=3)
    assert (r["f"], r["pred"], r["n_chains"]) == ([5, 8], [-1, -1], 2)
    # one more on the first anchor and it is one
    assert CR.chain_reference(*_cols([(0, 0, 6), (11, 14, 8)]), band=3)["pred"] == [-1, 0]


SECONDARY = [(0, 0, 10), (10, 10, 10), (20, 22, 10), (30, 20, 15)]   # ends (10,10) (20,20) (30,32) (45,35)


def test_secondary_chain_stops_at_a_taken_anchor():
    # 2 after 1: da 10, db 12: 20 + 10 - gc(2) = 26.  3 after 2: da 15, db 3, skew 12: 26 + 3 - 14 = 15; after 1: da 25,
    # db 15, skew 10: 20 + 15 - 12 = 23; after 0: 10 + 15 - 12 = 13.  Chains: 2 -> 1 -> 0 (26), then 3, which stops at
    # the taken 1: 23 - 20
    r = CR.chain_reference(*_cols(SECONDARY), band=20)
    assert (r["f"], r["pred"]) == ([10, 20, 26, 23], [-1, 0, 1, 1])
    assert (r["chain_of"], r["n_chains"], r["chain_score"]) == ([0, 0, 0, 1], 2, [26, 3])


def test_min_score_drops_a_chain_and_keeps_its_anchors_taken():
    r = CR.chain_reference(*_cols(SECONDARY), band=20, min_score=4)
    assert (r["chain_of"], r["n_chains"], r["chain_score"]) == ([0, 0, 0, -1], 1, [26])
    assert CR.chain_reference(*_cols(SECONDARY), band=20, min_score=3)["n_chains"] == 2
    # two short chains: the dropped one's first anchor does not start a chain of its own, and the ranks close up
    r = CR.chain_reference(*_cols([(0, 0, 3), (1, 1, 3), (50, 90, 9)]), band=0, min_score=5)
    assert (r["f"], r["pred"]) == ([3, 4, 9], [-1, 0, -1])
    assert (r["chain_of"], r["n_chains"], r["chain_score"]) == ([-1, -1, 0], 1, [9])


def test_any_order_and_the_plan():
    # the caller's order is not the sorted one: indices come back as the caller's
    a, b, ln = [30, 0, 12], [28, 0, 10], [10, 10, 5]   # ends (40, 38), (10, 10), (17, 15)
    assert CR.sort_order(a, b, ln) == [1, 2, 0]
    ch = CR.chains(a, b, ln, band=4)
    # 2 after 1: da 7, db 5: 10 + 5 - gc(2) = 11; 0 after 2: da = db = 23: 11 + 10 = 21
    assert ch == [dict(score=21, anchors=[1, 2, 0], a_beg=0, b_beg=0, a_end=40, b_end=38)]
    p = CR.plan(a, b, ln, ch[0]["anchors"])
    # anchor 2 keeps all 5 columns and leaves 2 symbols of A alone; anchor 0 keeps 10 of 10 behind a 13 x 13 region
    assert p == dict(left=(0, 0), right=(40, 38),
                     parts=[("seed", 0, 10, 0, 10), ("gap", 10, 12, 10, 10), ("seed", 12, 17, 10, 15),
                            ("gap", 17, 30, 15, 28), ("seed", 30, 40, 28, 38)])
    # duplicates are allowed and stay in the caller's order
    assert CR.sort_order([5, 5], [5, 5], [3, 3]) == [0, 1]
    assert CR.chain_reference([5, 5], [5, 5], [3, 3], band=0)["pred"] == [-1, -1]

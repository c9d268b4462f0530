"""The batch walk (msa_plan_traceback_batch: one wave per pair, every pair of a plan in one launch) and the host
batch entries (msa_sw_align_batch, msa_nw_align_batch) against the oracle (oracle.sw, oracle.banded_ref), the
numpy restatement in tests/nw_reference.py and the single-pair walkers.

Shapes are the smallest at which each mechanism of the walk kernel can fail: a 1 x 1 walk, a partial stripe, a
64-cell run, a single-row last stripe, more steps than one 256-step group, runs across stripe borders, long gaps
in both directions (a walk leaving its group on the left; stripes crossed in state F), a pair that is not walked,
a pair count that leaves idle waves in the last workgroup, ops at every byte alignment, and a pair with more
stripes than a walk stages start columns for."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import nw_reference as R
from nw_reference import rs, similar

pytestmark = pytest.mark.gpu

_TR = bytes.maketrans(b"ACGT", b"\x00\x01\x02\x03")
UNSUPPORTED, ARG, CAPACITY, ALPHABET = -5, -1, -8, -2
SW = dict(match=2, mismatch=-1, gap_open=3, gap_extend=1)


def enc(s: bytes) -> np.ndarray:
    return np.frombuffer(s.translate(_TR), dtype=np.uint8).copy()


def _dev(x, dev):
    import torch

    return torch.from_numpy(enc(x)).to(dev)


def _offs(lens):
    return [int(x) for x in np.concatenate(([0], np.cumsum(lens)[:-1]))]


@pytest.fixture(scope="module")
def LB():
    from cse305_parallel_sequence_alignment_amd import _lib

    return _lib


# ---- the inputs -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sw_pairs():
    """Batch (a): eleven pairs (not a multiple of the walks per workgroup)."""
    rng = np.random.default_rng(7001)
    p = [(b"A", b"A"), (rs(rng, 63), rs(rng, 70))]
    X = rs(rng, 64)
    p.append((X, X))
    p.append((rs(rng, 65), rs(rng, 300)))
    X = rs(rng, 193)
    p.append((X, X + rs(rng, 7)))
    g = np.random.default_rng(7301)
    X, Y, Z = rs(g, 400), rs(g, 400), rs(g, 300)
    p.append((X + Y, X + Z + Y))  # 6: a 300D gap
    T = rs(g, 350)
    p.append((X + Z + Y, X + Y + T))  # 7: a 300I gap
    g = np.random.default_rng(7600)
    X, Y, W = rs(g, 600), rs(g, 600), rs(g, 600)
    Z1, Z2 = rs(g, 300), rs(g, 300)
    p.append((X + Z1 + Y + W, X + Y + Z2 + W))  # 8: both
    p.append((b"A" * 100, b"C" * 90))  # 9: score 0
    p.append(similar(np.random.default_rng(31), 700))
    p.append((rs(rng, 130), rs(rng, 129)))
    assert len(p) == 11
    return tuple(p)


@functools.lru_cache(maxsize=None)
def split_pairs():
    """Batch (b): test_batch_split_pairs[affine_dir]'s five pairs."""
    rng = np.random.default_rng(3)
    As = [rs(rng, 1300) for _ in range(5)]
    Bs = [rs(rng, 1250) for _ in range(5)]
    return tuple(zip(As, Bs))


@functools.lru_cache(maxsize=None)
def nw_batches():
    """Batches (c): name -> (pairs, band); g = 1, h = 2."""
    return {
        "batch_w64": (tuple(R.batch_pairs()), 64),
        "batch_noband": (tuple(R.batch_pairs()), -1),
        "wide_w64": (tuple(R.batch_wide_pairs()), 64),
        "border_w40": ((R._border(False), R._border(True), R._rnd(13, 300, 290)), 40),
        "ties_w16": (((b"A" * 400, b"A" * 390), (b"A" * 300, b"C" * 300)), 16),
    }


@functools.lru_cache(maxsize=None)
def nw_refs(name):
    pairs, band = nw_batches()[name]
    return tuple(R.nw_reference(A, B, 1, 2, band) for A, B in pairs)


_ORC = {}


def sw_refs(oracle, key, pairs, sc):
    """The oracle's alignments of a batch, computed once and shared (never modified)."""
    if key not in _ORC:
        _ORC[key] = [oracle.sw(A, B, sc["match"], sc["mismatch"], sc["gap_open"], sc["gap_extend"], want_tb=True)
                     for A, B in pairs]
    return _ORC[key]


def _sw_fill(LB, dev, pairs, sc, **kw):
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    kw.setdefault("track_end", True)
    kw.setdefault("single", False)
    pl = Plan(LB.SW_AFFINE, LB.CELLS_DIR, ms, ns, _offs(ms), _offs(ns), **sc, **kw)
    D = torch.empty(pl.cells_elems, dtype=torch.uint8, device=dev)
    pl.run(_dev(b"".join(a for a, _ in pairs), dev), _dev(b"".join(b for _, b in pairs), dev), D)
    return pl, D


def _nw_fill(LB, dev, pairs, band, stream=None):
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    ms, ns = [len(a) for a, _ in pairs], [len(b) for _, b in pairs]
    pl = Plan(LB.NW_ALIGN, LB.CELLS_DIR, ms, ns, _offs(ms), _offs(ns), match=1, mismatch=0, gap_open=3, gap_extend=1,
              band=band)
    D = torch.zeros(pl.cells_elems, dtype=torch.uint8, device=dev)
    dA, dB = _dev(b"".join(a for a, _ in pairs), dev), _dev(b"".join(b for _, b in pairs), dev)
    torch.cuda.synchronize()
    pl.run(dA, dB, D, stream=stream)
    return pl, D


def _walk(pl, D, off, fill=0xEE):
    """One batch launch into a prefilled buffer: (ops bytes as numpy, info (n_pairs, 8))."""
    import torch

    dev = D.device
    ops = torch.full((max(off[-1], 1) + 64,), fill, dtype=torch.uint8, device=dev)
    info = torch.zeros(8 * len(pl.ms), dtype=torch.int64, device=dev)
    pl.traceback_batch_async(D, ops, torch.tensor(off, dtype=torch.int64, device=dev), info)
    return ops.cpu().numpy(), info.cpu().numpy().reshape(-1, 8)


def _untouched(buf, off, info, fill=0xEE):
    """Every byte outside [off[p], off[p] + min(n_ops, capacity)) still holds the fill."""
    free = np.ones(len(buf), dtype=bool)
    for p in range(len(off) - 1):
        free[off[p]:off[p] + min(int(info[p, 0]), off[p + 1] - off[p])] = False
    return bool((buf[free] == fill).all())


def _single_sw(pl, D, k):
    """The single walker on pair k: (ops, info[0..3])."""
    import torch

    ops = torch.empty(pl.ms[k] + pl.ns[k] + 2, dtype=torch.uint8, device=D.device)
    info = torch.zeros(8, dtype=torch.int64, device=D.device)
    pl.traceback_async(D, ops, info, pair=k)
    inf = info.cpu().tolist()
    return ops[:inf[0]].cpu().numpy().tobytes(), inf[:4]


def _check_sw_batch(pl, D, pairs, refs):
    from cse305_parallel_sequence_alignment_amd.plan import Plan, cigar_of

    res = pl.results()
    singles = [_single_sw(pl, D, k) for k in range(len(pairs))]
    tight = [0]
    for a, b in pairs:
        tight.append(tight[-1] + len(a) + len(b) + 1)  # unaligned: stores at any byte alignment
    for off in (Plan.ops_layout(pl.ms, pl.ns), tight):
        buf, info = _walk(pl, D, off)
        for k, o in enumerate(refs):
            assert (res[k]["score"], tuple(res[k]["end"])) == (o["score"], tuple(o["end"])), k
            ops = buf[off[k]:off[k] + int(info[k, 0])].tobytes()
            assert ops == singles[k][0], k
            assert info[k, :4].tolist() == singles[k][1], (k, info[k].tolist(), singles[k][1])
            assert info[k, 3] == 0, k
            assert (int(info[k, 1]), int(info[k, 2])) == tuple(o["beg"]), k
            assert cigar_of(ops) == o["cigar"], k
        assert _untouched(buf, off, info)
    assert pl.error() == 0
    # ... and the fetched form
    tb = pl.traceback_batch(D)
    assert [(t["ops"], t["beg"], t["cigar"]) for t in tb] == \
        [(s[0], (s[1][1], s[1][2]), o["cigar"]) for s, o in zip(singles, refs)]


# ---- a. SW walk, ragged batch -------------------------------------------------------------------------
def test_sw_ragged_batch(oracle, dev, LB):
    pairs = sw_pairs()
    refs = sw_refs(oracle, "a", pairs, SW)
    # the cases the batch is there for, asserted from the oracle's alignments
    assert refs[5]["score"] == 1298 and "300D" in refs[5]["cigar"] and "I" not in refs[5]["cigar"]
    assert refs[6]["score"] == 1298 and "300I" in refs[6]["cigar"] and "D" not in refs[6]["cigar"]
    assert refs[7]["score"] == 2996 and "300I" in refs[7]["cigar"] and "300D" in refs[7]["cigar"]
    assert refs[8]["score"] == 0 and refs[8]["cigar"] == ""
    assert refs[2]["cigar"] == "64M" and refs[0]["cigar"] == "1M"
    pl, D = _sw_fill(LB, dev, pairs, SW)
    assert pl.launch_info()["mode"] == "stripe"
    _check_sw_batch(pl, D, pairs, refs)
    assert pl.traceback_batch(D)[8]["ops"] == b""  # score 0: no walk


# ---- b. SW walk, split batch --------------------------------------------------------------------------
def test_sw_split_batch(oracle, dev, LB):
    sc = dict(match=1, mismatch=0, gap_open=3, gap_extend=1)
    pairs = split_pairs()
    pl, D = _sw_fill(LB, dev, pairs, sc)
    assert pl.launch_info()["mode"] == "split"
    _check_sw_batch(pl, D, pairs, sw_refs(oracle, "b", pairs, sc))


# ---- c. global walk -----------------------------------------------------------------------------------
def _check_nw_batch(oracle, pl, D, name, stream=None):
    pairs, band = nw_batches()[name]
    tb = pl.traceback_batch(D, stream=stream)
    res = pl.results(stream=stream)
    for k, ((A, B), ref) in enumerate(zip(pairs, nw_refs(name))):
        score = int(oracle.banded_ref(A, B, ref["w"], 1.0, 2.0))
        assert res[k]["score"] == ref["score"] == score, (name, k)
        assert tb[k]["ops"] == ref["ops"], (name, k)
        assert tb[k]["stop"] == ref["stop"], (name, k)
        assert tb[k]["cigar"] == R.cigar_of(ref["ops"]), (name, k)
        assert R.rescore(A, B, tb[k]["ops"], 1, 2, band) == score, (name, k)
        assert tb[k]["ops"] == pl.traceback_nw(D, pair=k, stream=stream)["ops"], (name, k)
    assert pl.error(stream=stream) == 0
    return tb


@pytest.mark.parametrize("name", ["batch_w64", "batch_noband", "wide_w64", "border_w40", "ties_w16"])
def test_nw_batch(oracle, dev, LB, name):
    pairs, band = nw_batches()[name]
    pl, D = _nw_fill(LB, dev, pairs, band)
    tb = _check_nw_batch(oracle, pl, D, name)
    if name == "border_w40":
        refs = nw_refs(name)
        assert [t["stop"] for t in tb] == [(25, 0), (0, 25), (0, 0)]
        assert [r["score"] for r in refs] == [348, 348, 89]
        assert tb[0]["cigar"].startswith("25I") and tb[1]["cigar"].startswith("25D")


def test_nw_more_stripes_than_staged_starts(oracle, dev, LB):
    """A pair of 516 stripes -- a walk stages 512 stripe start columns in LDS and reads the rest from the stripe
    meta -- beside a short one, band 64: the single walker's ops, which rescore to the oracle's score."""
    A, B = R._sim(41, 33000)
    assert (len(A) + 63) // 64 > 512 and abs(len(A) - len(B)) <= 64
    pairs = ((A, B), R._rnd(13, 300, 290))
    pl, D = _nw_fill(LB, dev, pairs, 64)
    tb = pl.traceback_batch(D)
    res = pl.results()
    for k, (a, b) in enumerate(pairs):
        score = int(oracle.banded_ref(a, b, 64, 1.0, 2.0))
        assert res[k]["score"] == score, k
        assert tb[k]["ops"] == pl.traceback_nw(D, pair=k)["ops"], k
        assert R.rescore(a, b, tb[k]["ops"], 1, 2, 64) == score, k
    assert tb[0]["stats"]["switches"] == 516
    assert pl.error() == 0


# ---- d. capacity --------------------------------------------------------------------------------------
def test_capacity(oracle, dev, LB):
    """Pair 10 gets 10 bytes and pair 2 none: both report MSA_ERR_CAPACITY and their true n_ops, nothing is written
    past either range, every other pair is complete."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan, cigar_of

    pairs = sw_pairs()
    refs = sw_refs(oracle, "a", pairs, SW)
    pl, D = _sw_fill(LB, dev, pairs, SW)
    full = Plan.ops_layout(pl.ms, pl.ns)
    caps = [b - a for a, b in zip(full, full[1:])]
    caps[9], caps[1] = 10, 0
    off = [0] + [int(x) for x in np.cumsum(caps)]
    buf, info = _walk(pl, D, off)
    want = [_single_sw(pl, D, k) for k in range(len(pairs))]
    for k in range(len(pairs)):
        assert int(info[k, 0]) == len(want[k][0]), k
        assert (int(info[k, 1]), int(info[k, 2])) == tuple(refs[k]["beg"]), k
        if k in (1, 9):
            assert info[k, 3] == CAPACITY and int(info[k, 0]) > caps[k], (k, info[k].tolist())
        else:
            assert info[k, 3] == 0, k
            ops = buf[off[k]:off[k] + int(info[k, 0])].tobytes()
            assert ops == want[k][0] and cigar_of(ops) == refs[k]["cigar"], k
    assert buf[off[9]:off[9] + 10].tobytes() == want[9][0][:10]
    assert _untouched(buf, off, info)
    with pytest.raises(LB.MsaError) as e:
        pl.traceback_batch(D, ops_off=off)
    assert e.value.status == CAPACITY


# ---- e. rejections ------------------------------------------------------------------------------------
def test_rejections(dev, LB):
    """Plans the batch walk does not take, and a NULL argument: the status, and nothing runs."""
    import torch
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    L, P = LB.lib(), lambda t: C.c_void_p(t.data_ptr())
    ops = torch.full((8192,), 0xEE, dtype=torch.uint8, device=dev)
    info = torch.full((64,), -77, dtype=torch.int64, device=dev)
    off = torch.tensor([0, 2048, 4096], dtype=torch.int64, device=dev)

    def call(pl, d_off=off):
        D = torch.zeros(max(pl.cells_elems, 16), dtype=torch.uint8 if pl.cells == LB.CELLS_DIR else torch.int32,
                        device=dev)
        return L.msa_plan_traceback_batch(pl._h, P(D), P(ops), None if d_off is None else P(d_off), P(info), None)

    flow = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [1500], [1400], [0], [0], track_end=True, single=True, **SW)
    assert flow.launch_info()["mode"] == "flow"
    assert call(flow) == UNSUPPORTED
    gotoh = Plan(LB.REF_GOTOH, LB.CELLS_DIR, [200], [190], [0], [0], match=1, mismatch=0, gap_open=3, gap_extend=1,
                 start_type=-1, single=False)
    assert call(gotoh) == UNSUPPORTED
    no_end = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [200, 150], [190, 160], [0, 200], [0, 190], track_end=False,
                  single=False, **SW)
    assert call(no_end) == UNSUPPORTED
    lin = Plan(LB.SW_LINEAR, LB.CELLS_H, [200, 150], [190, 160], [0, 200], [0, 190], match=2, mismatch=-1,
               gap_open=1, gap_extend=1, single=False)
    assert call(lin) == UNSUPPORTED
    ok = Plan(LB.SW_AFFINE, LB.CELLS_DIR, [200, 150], [190, 160], [0, 200], [0, 190], track_end=True, single=False,
              **SW)
    assert call(ok, d_off=None) == ARG
    torch.cuda.synchronize()
    assert bool((ops == 0xEE).all()) and bool((info == -77).all())  # nothing ran
    # the Python wrapper checks the offsets' shape before the call
    with pytest.raises(ValueError):
        ok.traceback_batch_async(torch.zeros(ok.cells_elems, dtype=torch.uint8, device=dev), ops, off[:2], info)


# ---- f. stream order ----------------------------------------------------------------------------------
def test_stream_order(oracle, dev, LB):
    """Run and batch walk on a non-default stream, no synchronise between them."""
    import torch

    s = torch.cuda.Stream(device=dev)
    pairs, band = nw_batches()["batch_w64"]
    pl, D = _nw_fill(LB, dev, pairs, band, stream=s)
    _check_nw_batch(oracle, pl, D, "batch_w64", stream=s)


# ---- g. host entries ----------------------------------------------------------------------------------
def _status(fn):
    from cse305_parallel_sequence_alignment_amd._lib import MsaError

    try:
        fn()
    except MsaError as e:
        return e.status
    return 0


def test_host_sw_batch(oracle, dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    pairs = sw_pairs()
    refs = sw_refs(oracle, "a", pairs, SW)
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    got = api.sw_align_batch(As, Bs, **SW)
    assert got == [api.sw_align(a, b, **SW) for a, b in pairs]
    assert got == [dict(score=o["score"], end=tuple(o["end"]), beg=tuple(o["beg"]), cigar=o["cigar"]) for o in refs]
    assert api.sw_align_batch(As, Bs, traceback=False, **SW) == [dict(score=g["score"], end=g["end"]) for g in got]


def test_host_nw_batch(oracle, dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    pairs, band = nw_batches()["batch_w64"]
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    got = api.nw_align_batch(As, Bs, gap_open=3, gap_extend=1, band=band)
    assert got == [api.nw_align(a, b, gap_open=3, gap_extend=1, band=band) for a, b in pairs]
    assert got == [dict(score=r["score"], cigar=R.cigar_of(r["ops"])) for r in nw_refs("batch_w64")]
    assert api.nw_align_batch(As, Bs, gap_open=3, gap_extend=1, band=band, traceback=False) == \
        [dict(score=g["score"]) for g in got]


def test_host_shared_reference(oracle, dev, LB):
    """Six mutated windows of one reference against the whole reference, given once."""
    from cse305_parallel_sequence_alignment_amd import api, data

    rng = np.random.default_rng(8101)
    ref = rs(rng, 2000)
    As = []
    for k in range(6):
        ln = int(rng.integers(300, 501))
        lo = int(rng.integers(0, 2000 - ln))
        As.append(data.mutate(ref[lo:lo + ln], 8200 + k))
    got = api.sw_align_batch(As, ref, **SW)
    assert got == [api.sw_align(a, ref, **SW) for a in As]
    for a, g in zip(As, got):
        o = oracle.sw(a, ref, SW["match"], SW["mismatch"], SW["gap_open"], SW["gap_extend"], want_tb=True)
        assert g == dict(score=o["score"], end=tuple(o["end"]), beg=tuple(o["beg"]), cigar=o["cigar"])
        assert g["score"] > len(a)  # (the windows do align)


def test_host_status(dev, LB):
    from cse305_parallel_sequence_alignment_amd import api

    # five symbols each, eight together: one map serves the call, SW takes seven
    assert _status(lambda: api.sw_align_batch([b"ACGTN" * 8, b"TNRYK" * 8], [b"ACGTN" * 7, b"TNRYK" * 7])) == ALPHABET
    A, B = R._rnd(12, 300, 310)
    assert _status(lambda: api.nw_align_batch([A, A], [B, B[:100]], band=64)) == ARG  # a pair outside the band
    assert _status(lambda: api.nw_align_batch([A], [B], gap_open=1, gap_extend=2)) == UNSUPPORTED
    # a range past its buffer
    L = LB.lib()
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    sc, coff, cig = (C.c_int32 * 2)(), i64(0, 0, 0), C.create_string_buffer(4096)
    args = (3, 1, -1, sc, cig, 4096, coff)
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 2, i64(0, 100), i64(200, 201), i64(0, 0), i64(300, 300),
                                *args) == ARG
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 2, i64(0, 100), i64(200, 200), i64(0, 11), i64(300, 300),
                                *args) == ARG
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 0, i64(0), i64(200), i64(0), i64(300), *args) == ARG
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 1, i64(0), i64(0), i64(0), i64(300), *args) == ARG
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 1, None, i64(200), i64(0), i64(300), *args) == ARG
    # a CIGAR buffer too small: the needed size comes back
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 1, i64(0), i64(300), i64(0), i64(310), 3, 1, -1, sc, cig, 2,
                                coff) == CAPACITY
    need = int(coff[1])
    assert L.msa_nw_align_batch(A, len(A), B, len(B), 1, i64(0), i64(300), i64(0), i64(310), 3, 1, -1, sc, cig,
                                need, coff) == 0
    assert cig.value.decode() == api.nw_align(A, B)["cigar"] and len(cig.value) + 1 == need


def test_host_threads(dev, LB):
    """Four threads run the same batch at once (each chunk is admitted against the device budget)."""
    from cse305_parallel_sequence_alignment_amd import api

    pairs, band = nw_batches()["batch_w64"]
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    want = [dict(score=r["score"], cigar=R.cigar_of(r["ops"])) for r in nw_refs("batch_w64")]
    out, errs = [None] * 4, []

    def work(k):
        try:
            out[k] = api.nw_align_batch(As, Bs, gap_open=3, gap_extend=1, band=band)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert all(o == want for o in out), out


def test_host_chunking(oracle, dev, LB):
    """A device budget small enough that batch (a) runs as several chunks (each admitted once): the same results."""
    from cse305_parallel_sequence_alignment_amd import api

    L = LB.lib()
    pairs = sw_pairs()
    As, Bs = [a for a, _ in pairs], [b for _, b in pairs]
    want = api.sw_align_batch(As, Bs, **SW)

    def admitted():
        v = (C.c_int64 * 5)()
        assert L.msa_device_budget_info(v) == 0
        return int(v[4])

    try:
        budget = 256 << 20  # (every pair's estimate holds a fixed pool slack)
        while True:
            assert L.msa_set_device_budget(budget) == 0
            before = admitted()
            got = api.sw_align_batch(As, Bs, **SW)
            chunks = admitted() - before
            if chunks >= 2:
                break
            budget //= 2
            assert budget >= 1 << 20, "the batch never split"
        assert got == want
    finally:
        L.msa_set_device_budget(0)

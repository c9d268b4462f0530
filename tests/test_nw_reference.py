"""The numpy restatement of banded global alignment with direction bytes (tests/nw_reference.py) against the
oracle's banded Gotoh (oracle/msa_oracle.c: orc_banded_ref2): the yardstick of tests/test_gpu_nw_align.py is
itself checked here, on the shapes that file runs.  No GPU."""
import numpy as np
import pytest

import nw_reference as R


def _check_ops(A, B, ref, band, g, h):
    assert R.rescore(A, B, ref["ops"], g, h, band) == ref["score"]
    i, j = ref["stop"]
    assert (i == 0 or j == 0) and ref["ops"].endswith(b"I" * i + b"D" * j)


@pytest.mark.parametrize("name", list(R.SMALL))
def test_small_shapes_match_banded_oracle(oracle, name):
    """Score and every in-band H cell equal the oracle's; the ops rescored give the score."""
    A, B, band, g, h = R.SMALL[name]()
    ref = R.nw_reference(A, B, g, h, band)
    w = ref["w"]
    score, Ho = oracle.banded_ref(A, B, w, float(g), float(h), want_h=True)
    assert ref["score"] == int(score)
    v = ref["valid"]
    assert np.array_equal(ref["H"][v], R.to_band(Ho, w)[v])
    assert R.digest_h(ref["H"], len(B), w) == oracle.checksum_h(Ho, w)
    # the byte's low bits are never 0 on an in-band interior cell
    assert ((ref["byte"][v] & 3) != 0).all()
    _check_ops(A, B, ref, band, g, h)


@pytest.mark.parametrize("name", list(R.CHUNKED))
def test_large_shapes_match_banded_oracle(oracle, name):
    """The two chunked inputs: score and the digest of every in-band H cell; the ops rescored give the score."""
    A, B, band, g, h = R.chunked_case(name)
    ref = R.nw_reference(A, B, g, h, band)
    score, digest = oracle.banded_ref(A, B, band, float(g), float(h), want_digest=True)
    assert ref["score"] == int(score)
    assert R.digest_h(ref["H"], len(B), band) == digest
    _check_ops(A, B, ref, band, g, h)


def test_batch_pairs_match_banded_oracle(oracle):
    for band, pairs in ((64, R.batch_pairs()), (-1, R.batch_pairs()), (R.BATCH_WIDE_BAND, R.batch_wide_pairs())):
        for A, B in pairs:
            ref = R.nw_reference(A, B, 1, 2, band)
            score, Ho = oracle.banded_ref(A, B, ref["w"], 1.0, 2.0, want_h=True)
            assert ref["score"] == int(score)
            assert np.array_equal(ref["H"][ref["valid"]], R.to_band(Ho, ref["w"])[ref["valid"]])
            _check_ops(A, B, ref, band, 1, 2)


def test_border_stops():
    """B = A[25:] (and the mirror): the walk stops on the border and the CIGAR starts with the border gap."""
    for name, stop, lead in (("border_25I_w40", (25, 0), "25I"), ("border_25D_w40", (0, 25), "25D")):
        A, B, band, g, h = R.SMALL[name]()
        ref = R.nw_reference(A, B, g, h, band)
        assert ref["stop"] == stop and R.cigar_of(ref["ops"]).startswith(lead), (ref["stop"], R.cigar_of(ref["ops"])[:20])


def test_rescore_rejects_bad_ops():
    A, B = b"ACGTACGT", b"ACGACGT"
    assert R.rescore(A, B, b"MMMIMMMM"[::-1], 1, 2, 1) == 7 - 1 - 2  # ACG, T against a gap, ACGT
    with pytest.raises(AssertionError):
        R.rescore(A, B, b"MMMMMMM", 1, 2, 1)  # does not consume A
    with pytest.raises(AssertionError):
        R.rescore(A, B, b"IIIIIIII" + b"DDDDDDD", 1, 2, 3)  # leaves the band

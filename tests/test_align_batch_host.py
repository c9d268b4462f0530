"""Host side of the batch walk and the batch entries (msa_plan_traceback_batch, msa_sw_align_batch,
msa_nw_align_batch): the pure layout helper, the empty batch, the exported symbols, and the no-device status.
Nothing here needs a GPU."""
import ctypes as C

import pytest

NEW = ("msa_plan_traceback_batch", "msa_sw_align_batch", "msa_nw_align_batch")


def test_ops_layout():
    """off[0] = 0, off[p+1] = off[p] + round_up(m_p + n_p + 2, 16); static and pure (no plan, no library)."""
    from cse305_parallel_sequence_alignment_amd.plan import Plan

    assert Plan.ops_layout([1, 63], [1, 70]) == [0, 16, 160]  # 1+1+2 -> 16; 63+70+2 = 135 -> 144
    assert Plan.ops_layout([], []) == [0]
    assert Plan.ops_layout([7], [7]) == [0, 16]  # exactly 16
    assert Plan.ops_layout([8], [7]) == [0, 32]


def test_empty_batch_returns_empty_list(monkeypatch):
    """Empty input returns [] without touching the library."""
    from cse305_parallel_sequence_alignment_amd import _lib, api

    def boom():
        raise AssertionError("the library was loaded for an empty batch")

    monkeypatch.setattr(_lib, "lib", boom)
    assert api.sw_align_batch([], []) == []
    assert api.nw_align_batch([], []) == []
    assert api.sw_align_batch([], b"ACGT") == []


def test_new_symbols_exported():
    from cse305_parallel_sequence_alignment_amd import _lib as LB

    L = LB.lib()
    for name in NEW:
        assert name in LB.EXPORTED
        assert hasattr(L, name), f"libmsa.so does not export {name}"


def test_batch_list_lengths_checked():
    from cse305_parallel_sequence_alignment_amd import api

    with pytest.raises(ValueError):
        api.nw_align_batch([b"ACGT", b"ACG"], [b"ACGT"])


def test_no_device_status():
    """Without a GPU a valid batch call returns MSA_ERR_NODEV (no fallback)."""
    from cse305_parallel_sequence_alignment_amd import _lib as LB, api

    n = C.c_int(0)
    if LB.lib().msa_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(LB.MsaError) as e:
        api.nw_align_batch([b"ACGT"], [b"ACGT"])
    assert e.value.status == -4
    with pytest.raises(LB.MsaError) as e:
        api.sw_align_batch([b"ACGT"], b"ACGT")
    assert e.value.status == -4

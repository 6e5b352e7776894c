"""The device suffix pre-sort (gmx_suffixsort.hip) pinned on crafted raw texts (tests/suffix_common.py).

Its contract, checked on its own through gmx_debug_suffix_presort — before the host repair, which would hide a pre-sort that
marks too few ties wherever stable radix order happens to agree with suffix order: `sa` is a permutation ordered by (K1, K2),
and bit p of the mask is set exactly when sa[p] agrees with sa[p - 1] on both keys. Then the whole forced device route against
a plain suffix sort, the documented fall-back on a text the repair gives up on, and the piecewise scans (exclusive_sum,
running_max_in_place) with the piece shrunk by GMX_SORT_SCAN_PIECE so that their carry runs on 70 000 symbols."""
import numpy as np
import pytest

from gramtools_amd import _lib
from suffix_common import (ROUTE_VARIABLES, SCAN_PIECES, crafted_texts, fallback_text, keys, plain_of, presort, suffix_array)

pytestmark = pytest.mark.gpu

A_TO_G = crafted_texts("abcdefg")
H = crafted_texts("h")


@pytest.fixture
def lib(monkeypatch):
    for name in ROUTE_VARIABLES:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def _check_contract(text, sa, bits):
    n = text.size
    k1, _, k2 = keys(text)
    assert np.array_equal(np.sort(sa), np.arange(n, dtype=np.uint32))
    a, b = sa[:-1], sa[1:]
    assert (k1[a] <= k1[b]).all()
    same1 = k1[a] == k1[b]
    assert (k2[a][same1] <= k2[b][same1]).all()
    want = np.zeros(bits.size, dtype=np.uint8)
    want[1:n] = same1 & (k2[a] == k2[b])
    missing = np.flatnonzero((want == 1) & (bits == 0))
    extra = np.flatnonzero((want == 0) & (bits == 1))   # (bits at or past n among them)
    assert missing.size == 0 and extra.size == 0, (missing[:8].tolist(), extra[:8].tolist())
    return int(want.sum())


@pytest.mark.parametrize("name,text", A_TO_G, ids=[n for n, _ in A_TO_G])
def test_presort_orders_by_both_keys_and_marks_exactly_the_ties(lib, name, text):
    rc, sa, bits = presort(lib, text)
    assert rc == 0, lib.gmx_last_error()
    tied = _check_contract(text, sa, bits)
    if name == "d-distinct-markers":   # no two keys equal: the second round is skipped
        assert tied == 0 and not bits.any()


@pytest.mark.parametrize("name,text", A_TO_G, ids=[n for n, _ in A_TO_G])
def test_forced_device_route_equals_the_plain_sort(lib, monkeypatch, name, text):
    monkeypatch.setenv("GMX_DEVICE_BUILD", "1")   # (an error if the device sort cannot be used: that it ran is part of the result)
    rc, got = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    assert np.array_equal(got, plain_of(name))


def test_a_text_the_repair_gives_up_on_is_an_error_or_falls_back(lib, monkeypatch):
    text = fallback_text()
    monkeypatch.setenv("GMX_SAIS", "1")
    rc, want = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    monkeypatch.delenv("GMX_SAIS")
    monkeypatch.setenv("GMX_DEVICE_BUILD", "1")
    rc, _ = suffix_array(lib, text, threads=4)
    assert rc == -1 and b"could not be used" in lib.gmx_last_error()
    monkeypatch.setenv("GMX_DEVICE_SORT_MAY_FALL_BACK", "1")
    rc, got = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    assert np.array_equal(got, want)


_whole_piece = {}   # name -> (sa, bits, finished array by SA-IS), computed once with the piece unset


def _baseline(lib, monkeypatch, name, text):
    if name not in _whole_piece:
        rc, sa, bits = presort(lib, text)
        assert rc == 0, lib.gmx_last_error()
        _check_contract(text, sa, bits)
        monkeypatch.setenv("GMX_SAIS", "1")
        rc, want = suffix_array(lib, text, threads=4)
        monkeypatch.delenv("GMX_SAIS")
        assert rc == 0, lib.gmx_last_error()
        for a in (sa, bits, want):
            a.setflags(write=False)
        _whole_piece[name] = (sa, bits, want)
    return _whole_piece[name]


@pytest.mark.parametrize("piece", SCAN_PIECES)
@pytest.mark.parametrize("name,text", H, ids=[n for n, _ in H])
def test_scans_cut_into_pieces_give_the_same_presort(lib, monkeypatch, name, text, piece):
    sa0, bits0, want = _baseline(lib, monkeypatch, name, text)
    monkeypatch.setenv("GMX_SORT_SCAN_PIECE", str(piece))
    rc, sa, bits = presort(lib, text)
    assert rc == 0, lib.gmx_last_error()
    assert sa.tobytes() == sa0.tobytes() and bits.tobytes() == bits0.tobytes()
    monkeypatch.setenv("GMX_DEVICE_BUILD", "1")
    rc, got = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    assert np.array_equal(got, want)

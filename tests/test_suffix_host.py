"""The suffix-array builder's host routes on crafted raw texts (tests/suffix_common.py), and the restated key of the device
pre-sort against a plain suffix sort: the reference tests/test_suffix_presort.py leans on. No GPU."""
import numpy as np
import pytest

from gramtools_amd import _lib
from suffix_common import ROUTE_VARIABLES, crafted_texts, keys, plain_of, suffix_array

A_TO_G = crafted_texts("abcdefg")
H = crafted_texts("h")


@pytest.fixture
def lib(monkeypatch):
    for name in ROUTE_VARIABLES:
        monkeypatch.delenv(name, raising=False)
    return _lib.load()


def _still_tied_in_wrong_order(text, sa):
    """Pairs of neighbours in the true array that agree on both keys and stand in descending index order."""
    k1, _, k2 = keys(text)
    a, b = sa[:-1], sa[1:]
    return int(((k1[a] == k1[b]) & (k2[a] == k2[b]) & (a > b)).sum())


@pytest.mark.parametrize("name,text", A_TO_G, ids=[n for n, _ in A_TO_G])
def test_restated_keys_never_contradict_the_plain_sort(name, text):
    k1, length, k2 = keys(text)
    sa = plain_of(name)
    assert sorted(sa.tolist()) == list(range(text.size))
    a, b = sa[:-1], sa[1:]
    assert (k1[a] <= k1[b]).all()
    same = k1[a] == k1[b]
    assert (k2[a][same] <= k2[b][same]).all()
    assert (length[a][same] == length[b][same]).all()
    assert ((length >= 1) & (length <= 12)).all()
    # what the families promise
    tied = int((same & (k2[a] == k2[b])).sum())
    if name.startswith("b-") or name in ("d-marker-runs", "d-alternating"):
        assert _still_tied_in_wrong_order(text, sa) > 0
    if name.startswith("c-copies-"):
        L = int(name.rsplit("-", 1)[1])
        first, second = 17, 17 + L + 1 + 29
        assert (text[first:first + L] == text[second:second + L]).all() and text[first + L] == 4 and text[second + L] == 1
        pos = np.empty(text.size, dtype=np.int64)
        pos[sa] = np.arange(text.size)
        assert pos[second] < pos[first]
        both = k1[first] == k1[second] and k2[first] == k2[second]
        assert both == (L >= 24)
        if L >= 24:
            assert _still_tied_in_wrong_order(text, sa) > 0
    if name.endswith("-neighbour-groups"):
        # among the elements the second round sees (first key shared), neighbours of different groups with equal second keys
        _, inverse, counts = np.unique(k1, return_inverse=True, return_counts=True)
        seen = sa[counts[inverse][sa] > 1]
        a2, b2 = seen[:-1], seen[1:]
        assert ((k1[a2] != k1[b2]) & (k2[a2] == k2[b2])).any()
    if name == "d-distinct-markers":
        assert np.unique(k1).size == text.size and (length == 1).all()
    if name == "g-dense":
        _, counts = np.unique(k1, return_counts=True)   # 4096 possible keys: most suffixes share theirs
        assert tied == 0 and int(counts[counts > 1].sum()) > text.size // 2
    if name == "g-dense-copies":
        assert tied >= 3 * (60 - 24)


@pytest.mark.parametrize("name,text", A_TO_G, ids=[n for n, _ in A_TO_G])
def test_host_routes_equal_the_plain_sort(lib, monkeypatch, name, text):
    want = plain_of(name)
    monkeypatch.setenv("GMX_SAIS", "1")
    rc, got = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    assert np.array_equal(got, want)
    monkeypatch.delenv("GMX_SAIS")
    monkeypatch.setenv("GMX_PSORT_MIN", "1")
    rc, got = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name,text", H, ids=[n for n, _ in H])
def test_host_routes_agree_on_the_scan_piece_texts(lib, monkeypatch, name, text):
    monkeypatch.setenv("GMX_SAIS", "1")
    rc, sais = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    monkeypatch.delenv("GMX_SAIS")
    monkeypatch.setenv("GMX_PSORT_MIN", "1")
    rc, psort = suffix_array(lib, text, threads=4)
    assert rc == 0, lib.gmx_last_error()
    assert np.array_equal(sais, psort)
    assert np.array_equal(np.sort(sais), np.arange(text.size, dtype=np.uint32))


def test_builder_errors_come_back_as_einval(lib):
    rc, _ = suffix_array(lib, np.array([1, 2, 3], dtype=np.uint32))
    assert rc == -1 and b"must end with the sentinel" in lib.gmx_last_error()
    rc, _ = suffix_array(lib, np.array([1, 0, 2, 0], dtype=np.uint32))
    assert rc == -1 and b"sentinel 0 inside" in lib.gmx_last_error()
    assert lib.gmx_debug_suffix_array_u32(None, 4, 1, None) == -1
    assert lib.gmx_debug_suffix_presort(None, 4, None, None) == -1

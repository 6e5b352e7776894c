"""Crafted raw texts for the suffix-array builder, a plain reference sort, and the device pre-sort's key restated.

gmx_suffixsort.hip orders the suffixes by two 12-symbol keys and marks what still ties; gmx_index.cpp finishes those runs by
comparison. The texts here are chosen for the places where that can go wrong — key ends at 12 and 24 symbols, keys cut short by
markers, the 28-bit marker field, tie groups whose index order is not suffix order, no ties at all, texts shorter than one key,
scans cut into pieces — and most of them are no valid PRG, so they go through the raw-text hooks gmx_debug_suffix_array_u32 and
gmx_debug_suffix_presort. Everything in this module is numpy / Python; tests/test_suffix_host.py checks it against itself.
"""
import ctypes as C
import functools
import itertools

import numpy as np

KEY_SYMBOLS = 12
SCAN_PIECES = (1000, 4096, 65536)   # GMX_SORT_SCAN_PIECE values of the piece tests
ROUTE_VARIABLES = ("GMX_SAIS", "GMX_PSORT_MIN", "GMX_DEVICE_BUILD", "GMX_NO_DEVICE_SORT", "GMX_DEVICE_SORT_MAY_FALL_BACK",
                   "GMX_SORT_SCAN_PIECE")


def plain_suffix_array(text):
    """The suffix array by sorting the suffixes as byte strings (big-endian 4-byte symbols compare like the symbols)."""
    text = np.asarray(text, dtype=np.uint32)
    raw = text.astype(">u4").tobytes()
    return np.asarray(sorted(range(text.size), key=lambda i: raw[4 * i:]), dtype=np.uint32)


def keys(text):
    """suffix_key of gmx_suffixsort.hip's header, restated: up to 12 symbols of 3 bits each (sentinel 0, bases 1..4, marker 5),
    ending at and including the first marker or the sentinel, zero-padded, then 28 bits of that marker's value - 4.
    Returns K1[i], len[i] and K2[i] = K1[i + len[i]] (0 past the end)."""
    text = np.asarray(text, dtype=np.uint32)
    n = text.size
    digit = np.where(text == 0, 0, np.where(text <= 4, text, 5)).astype(np.uint64)
    dpad = np.concatenate([digit, np.zeros(KEY_SYMBOLS, dtype=np.uint64)])
    tpad = np.concatenate([text.astype(np.uint64), np.zeros(KEY_SYMBOLS, dtype=np.uint64)])
    key = np.zeros(n, dtype=np.uint64)
    marker = np.zeros(n, dtype=np.uint64)
    length = np.zeros(n, dtype=np.int64)
    open_ = np.ones(n, dtype=bool)
    at = np.arange(n)
    for j in range(KEY_SYMBOLS):
        take = open_ & (at + j < n)
        d = dpad[at + j]
        key = np.where(take, (key << np.uint64(3)) | d, key)
        length += take
        is_marker = take & (d == 5)
        marker = np.where(is_marker, tpad[at + j] - np.uint64(4), marker)
        open_ = take & (d != 0) & (d != 5)
    key = key << (np.uint64(3) * (KEY_SYMBOLS - length).astype(np.uint64))
    k1 = (key << np.uint64(28)) | marker
    nxt = at + length
    k2 = np.where(nxt < n, k1[np.minimum(nxt, n - 1)], np.uint64(0))
    return k1, length, k2


def _bases(rng, n, alphabet=4):
    return rng.integers(1, alphabet + 1, size=n, dtype=np.uint32)


def _text(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint32).reshape(-1) for p in parts] + [np.zeros(1, dtype=np.uint32)])


def _with_copies(text, rng, n_copies=3, seg=60):
    """`text` with `n_copies` segments of `seg` symbols copied to other places (the sentinel stays)."""
    text = text.copy()
    n = text.size - 1
    slots = rng.permutation(n // (2 * seg))[:2 * n_copies] * (2 * seg)   # disjoint places
    for src, dst in zip(slots[:n_copies], slots[n_copies:]):
        text[dst:dst + seg] = text[src:src + seg]
    return text


def _tied_after_both_rounds(text):
    k1, _, k2 = keys(text)
    pair = np.stack([k1, k2], axis=1)
    return text.size - np.unique(pair, axis=0).shape[0]


def _group_across_a_cut(text, piece):
    """Some group of equal first keys lies across a multiple of `piece` in sorted order (true where n has no such cut: the
    running maximum over n entries is then one piece)."""
    k1 = np.sort(keys(text)[0])
    cuts = np.arange(piece, text.size, piece)
    return cuts.size == 0 or bool((k1[cuts - 1] == k1[cuts]).any())


@functools.lru_cache(maxsize=None)
def _crafted():
    out = []   # (family, name, text)
    rng = np.random.default_rng(20240611)
    # a. shorter than one key, and around the ends of the first and the second key
    for n in (1, 2, 3, 11, 12, 13, 23, 24, 25, 26):
        out.append(("a", f"a-short-{n}", _text(_bases(rng, n - 1))))
    # b. periodic: every suffix ties past 24 symbols with the one a period later, which is the smaller (it meets the sentinel first)
    for p in (1, 2, 3, 4, 6, 11, 12, 13, 23, 24, 25):
        period = _bases(rng, p)
        out.append(("b", f"b-period-{p}", _text(np.tile(period, 599 // p + 1)[:599])))
    # c. two copies of a segment, the first followed by 4 and the second by 1: the later copy sorts first
    for L in (11, 12, 13, 23, 24, 25, 26, 40):
        seg = _bases(rng, L)
        out.append(("c", f"c-copies-{L}", _text(_bases(rng, 17), seg, [4], _bases(rng, 29), seg, [1], _bases(rng, 13))))
    # (c, d) neighbouring first-round groups whose second keys are equal: 1^12 and 1^11 2 before the same 12 bases, markers 6
    # and 7 before the same marker — a tie only if the group is left out of the comparison
    follow = np.concatenate([[3], _bases(rng, 11)]).astype(np.uint32)
    parts = []
    for i in range(4):
        parts += [[4, 3], [1] * 11, [1 + i % 2], follow, [2 + i % 3, 4]]
    out.append(("c", "c-neighbour-groups", _text(*parts)))
    out.append(("d", "d-neighbour-groups", _text([6, 9, 7, 9, 6, 9, 7, 9, 1, 7, 9, 2, 6, 9, 3])))
    # d. marker-dense
    out.append(("d", "d-marker-runs", _text([1, 2], [6] * 30, [3], [8] * 30, [2, 1], [6] * 30, [4], [1 << 20] * 30, [1])))
    out.append(("d", "d-alternating", _text(np.tile(np.array([5, 1, 6, 2, 6, 5], dtype=np.uint32), 40))))
    out.append(("d", "d-distinct-markers", _text(rng.permutation(np.arange(5, 5 + 300, dtype=np.uint32)))))
    # e. a marker in slot 11, in slot 12 (the first key's last) and in the second key's first slot, after the same 11 bases
    head = _bases(rng, 11)
    parts = []
    markers = iter((7, 8, 9, 41, 5, 1000003))
    for extra in (0, 1, 2, 0, 1, 2):
        parts += [head, np.array([2, 3], dtype=np.uint32)[:extra], [next(markers)], _bases(rng, 5)]
    out.append(("e", "e-marker-at-key-edge", _text(*parts)))
    # f. the marker field: the order of the blocks is decided by the 28 low bits alone
    values = [5, 6, 5 + (1 << 27), (1 << 28) - 2, (1 << 28) - 1]
    parts = []
    for v in (values[i] for i in (3, 0, 4, 2, 1, 0, 3)):
        parts += [[1, 2, 3, v], _bases(rng, 2)]
    out.append(("f", "f-marker-field", _text(*parts)))
    out.append(("f", "f-symbol-2^28", _text(*parts, [1, 2, 3, 1 << 28], _bases(rng, 2))))   # the builder sorts this one on the host
    # g. dense ties: 5000 symbols over {1, 2}; nearly every key ties in round 1, none after round 2 (a seed for which that holds)
    for seed in itertools.count(1):
        dense = _text(_bases(np.random.default_rng(seed), 4999, 2))
        if _tied_after_both_rounds(dense) == 0:
            break
    out.append(("g", "g-dense", dense))
    out.append(("g", "g-dense-copies", _with_copies(dense, rng)))
    # h. scan pieces: n = 65 536 (the n + 1-entry sum then has a last piece of one item at piece 65 536), n a multiple of the
    # other pieces, and one n that is no multiple of anything
    # (with one cut only, at 65 536, a group lies across it for most texts but not for all: the first seed for which one does)
    for n in (65536, 17 * 4096, 70000, 70001):
        for seed in itertools.count(n):
            r = np.random.default_rng(seed)
            text = _with_copies(_text(_bases(r, n - 1, 2)), r)
            if all(_group_across_a_cut(text, piece) for piece in SCAN_PIECES):
                break
        out.append(("h", f"h-pieces-{n}", text))
    for family, name, text in out:
        assert text.dtype == np.uint32 and text[-1] == 0 and (text[:-1] != 0).all(), name
        assert int(text.max()) < (1 << 28) or name == "f-symbol-2^28", name
        text.setflags(write=False)
    # the carry of the piecewise scans is exercised only where a round-1 group lies across a piece boundary in sorted order
    for family, name, text in out:
        if family != "h":
            continue
        for piece in SCAN_PIECES:
            assert _group_across_a_cut(text, piece), (name, piece)
            assert text.size + 1 > piece, (name, piece)   # the n + 1-entry sum has more than one piece
    return tuple(out)


def crafted_texts(families="abcdefg"):
    """[(name, text)] of the families asked for; each text ends with its only 0 and is read-only."""
    return [(name, text) for family, name, text in _crafted() if family in families]


def fallback_text():
    """Period 4, 20 000 symbols: the comparisons of finish_tied_runs exceed its budget of 400 n + 2^24."""
    return _text(np.tile(np.array([1, 2, 3, 4], dtype=np.uint32), 5000)[:19999])


@functools.lru_cache(maxsize=None)
def plain_of(name):
    """plain_suffix_array of a crafted text, computed once (read-only)."""
    sa = plain_suffix_array(dict(crafted_texts("abcdefgh"))[name])
    sa.setflags(write=False)
    return sa


# ---- the two hooks --------------------------------------------------------------------------------------------------
_u32p = C.POINTER(C.c_uint32)


def suffix_array(lib, text, threads=4):
    """gmx_debug_suffix_array_u32: (return code, array)."""
    text = np.ascontiguousarray(text, dtype=np.uint32)
    out = np.full(text.size, 0xFFFFFFFF, dtype=np.uint32)
    rc = lib.gmx_debug_suffix_array_u32(text.ctypes.data_as(_u32p), text.size, threads, out.ctypes.data_as(_u32p))
    return rc, out


def presort(lib, text):
    """gmx_debug_suffix_presort: (return code, sa, mask bits as one 0/1 byte per position, (n + 31) / 32 * 32 of them)."""
    text = np.ascontiguousarray(text, dtype=np.uint32)
    sa = np.full(text.size, 0xFFFFFFFF, dtype=np.uint32)
    words = np.full((text.size + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)
    rc = lib.gmx_debug_suffix_presort(text.ctypes.data_as(_u32p), text.size, sa.ctypes.data_as(_u32p), words.ctypes.data_as(_u32p))
    bits = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")
    return rc, sa, bits

"""tests/deflate_craft.py and the streams of tests/deflate_cases.py against zlib's inflater (no GPU): every valid stream the
device tests use inflates to expand(tokens), every invalid one is refused by zlib (or left incomplete, where the damage is a
truncation). A wrong helper would otherwise show as false failures, or false passes, of tests/test_inflate_crafted.py."""
import time
import zlib

import numpy as np
import pytest

import deflate_cases as cases
from deflate_craft import (Deflate, Match, expand, length_symbol, distance_symbol, gzip_member, bgzf_member, bgzf_file, limited_lengths, kraft,
                           greedy_cl_ops, expand_cl_ops)


def inflate(deflate_bytes):
    d = zlib.decompressobj(-15)
    return d.decompress(deflate_bytes), d


@pytest.mark.parametrize("case", cases.VALID, ids=repr)
def test_valid_streams_inflate_to_the_expanded_tokens(case):
    text, d = inflate(case.deflate)
    assert d.eof and d.unused_data == b""
    assert text == case.text
    assert zlib.decompress(gzip_member(case.deflate, case.text), 31) == case.text
    if "bgzf" in case.routes:
        assert len(case.text) <= 65536
        assert zlib.decompress(bgzf_member(case.deflate, case.text), 31) == case.text


@pytest.mark.parametrize("case", cases.INVALID, ids=repr)
def test_invalid_streams_are_refused_by_zlib(case):
    assert case.guard, "every damaged stream names the test of gmx_ingest.hip that refuses it"
    try:
        text, d = inflate(case.deflate + case.tail)
    except zlib.error:
        assert not case.trunc
        return
    if case.trunc:
        assert not d.eof
        return
    assert d.eof  # the deflate data is sound: the damage is in the member around it
    if case.tail:
        assert d.unused_data == case.tail
    with pytest.raises(zlib.error):
        zlib.decompress(gzip_member(case.deflate + case.tail, case.text, crc=case.crc, isize=case.isize), 31)


def test_random_streams_equal_zlib():
    rnd = cases.RANDOM()
    assert len(rnd) == 300
    kinds = set()
    for i, case in enumerate(rnd):
        text, d = inflate(case.deflate)
        assert d.eof and text == case.text, f"seed {cases.RANDOM_SEED}, member {i}"
        assert 500 <= len(text) <= 8192
        kinds.add(case.deflate[0] >> 1 & 3)
    assert kinds == {0, 1, 2}


def test_random_gzip_members_equal_zlib():
    """The members of the gzip route's random test: the same 300 specifications, three to a member."""
    members = cases.RANDOM_GZIP()
    assert len(members) == 100
    assert b"".join(c.text for c in members) == b"".join(c.text for c in cases.RANDOM())
    for i, case in enumerate(members):
        text, d = inflate(case.deflate)
        assert d.eof and d.unused_data == b"" and text == case.text, f"seed {cases.RANDOM_SEED}, member {i}"
        assert zlib.decompress(gzip_member(case.deflate, case.text), 31) == case.text


@pytest.mark.parametrize("printable", [True, False])
def test_piece_front_streams(printable):
    data, text, cuts = cases.piece_front_stream(printable)
    assert zlib.decompress(data, 31) == text
    assert 0 < cuts[0] < cuts[1] < len(data)
    allowed = set(cases.PRINTABLE if printable else cases.BINARY)
    assert set(text) <= allowed and (printable or not set(text) & set(cases.PRINTABLE))


def test_tables_are_the_rfcs():
    for ln in range(3, 259):
        s, e, v = length_symbol(ln)
        assert 257 <= s <= 285 and 0 <= v < (1 << e) or (e == 0 and v == 0)
    assert length_symbol(3) == (257, 0, 0) and length_symbol(10) == (264, 0, 0) and length_symbol(11) == (265, 1, 0)
    assert length_symbol(257) == (284, 5, 30) and length_symbol(258) == (285, 0, 0) and length_symbol(227) == (284, 5, 0)
    assert distance_symbol(1) == (0, 0, 0) and distance_symbol(4) == (3, 0, 0) and distance_symbol(5) == (4, 1, 0)
    assert distance_symbol(24577) == (29, 13, 0) and distance_symbol(32768) == (29, 13, 8191) and distance_symbol(24576) == (28, 13, 8191)
    # every length and distance, through zlib
    front = bytes(range(256)) * 128
    toks = [Match(ln, 1 + ln) for ln in range(3, 259)]
    d = Deflate().stored(front).fixed(toks, True)
    assert inflate(d.getvalue())[0] == d.text()
    for lo in range(1, 32769, 4096):
        d = Deflate().stored(front).fixed([Match(3, dist) for dist in range(lo, lo + 4096)], True)
        assert inflate(d.getvalue())[0] == d.text()


def test_expand_and_the_helpers_checks():
    assert expand([97, 98, (5, 2)]) == b"abababa" and expand([97, (4, 1)]) == b"aaaaa"
    with pytest.raises(ValueError):
        expand([97, (3, 2)])
    with pytest.raises(ValueError):
        Deflate().dynamic([97], True, lit_lens=[0] * 97 + [1] + [0] * 159, dist_lens=[0])        # no code for the end of the block
    with pytest.raises(ValueError):
        Deflate().dynamic([97, 98], True, lit_lens=cases.lens_of(257, {97: 1, 98: 2, 256: 3}), dist_lens=[0])  # incomplete
    with pytest.raises(ValueError):
        Deflate().dynamic([97, (3, 1)], True, dist_lens=[0])                                    # a distance symbol without a code
    with pytest.raises(ValueError):
        Deflate().dynamic([97], True, lit_lens=cases.lens_of(257, {97: 1, 256: 1}), dist_lens=[0], cl_ops=[(18, 97), 1, (18, 138), (18, 20), 1])
    rng = np.random.default_rng(1)
    for limit, n in ((15, 286), (7, 19), (15, 30)):
        for _ in range(50):
            f = (rng.random(n) ** 8 * 1e6).astype(int) * (rng.random(n) < 0.7)
            lens = limited_lengths(list(f), limit)
            used = int((f > 0).sum())
            assert max(lens) <= limit and all((l > 0) == (x > 0) for l, x in zip(lens, f))
            assert used < 2 or kraft(lens) == 1 << 15
            lens = cases.deepen(lens, rng, 30)
            assert used < 2 or (kraft(lens) == 1 << 15 and max(lens) <= 15)
            assert expand_cl_ops(greedy_cl_ops(lens)) == lens


def test_members_list_has_the_form_of_bgzf_members():
    from gramtools_amd import bgzf_members
    texts = [b"first member\n", b"the second\n" * 50]
    ms = [bgzf_member(Deflate().fixed(list(t), True).getvalue(), t) for t in texts]
    data, lst = bgzf_file(ms)
    assert lst == bgzf_members(data)
    assert [zlib.decompress(data[o:o + s], -15) for o, s, _, _ in lst] == texts


def test_the_writer_is_fast_enough():
    toks = list(np.random.default_rng(2).integers(0, 256, 65536))
    toks = [int(t) for t in toks]
    best = None
    for _ in range(3):  # (the best of three: a loaded host must not fail this)
        t0 = time.perf_counter()
        d = Deflate().dynamic(toks, True)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert inflate(d.getvalue())[0] == bytes(toks)
    assert best < 1.0, best

"""The device inflaters (gmx_ingest.hip: ing_inflate_member for BGZF members, gz_decode and the link / window / resolve kernels
for plain gzip) on deflate streams written by hand (tests/deflate_craft.py, the lists of tests/deflate_cases.py): what RFC 1951
allows and zlib's compressor never emits. The text must equal expand(tokens) byte for byte (tests/test_deflate_craft_host.py
pins the same streams to zlib's inflater, without a GPU), member CRCs are checked on the device, and damaged streams are
reported, never decoded. Many members go into one submit: one wavefront decodes one member."""
import pytest

import deflate_cases as cases
from deflate_craft import bgzf_member, bgzf_file, gzip_member, padded_header, GZ_HDR
from test_ingest_gzip import decode

pytestmark = pytest.mark.gpu

BAD_RECORD, BAD_MEMBER, BAD_CRC, TOO_MANY_LINES = 1, 2, 4, 8
NOT_FASTQ = BAD_RECORD | TOO_MANY_LINES  # the record scan's: the texts here are no FASTQ


@pytest.fixture
def pieces(monkeypatch):
    def set_(n):
        monkeypatch.setenv("GMX_GZ_PIECE", str(n))
    return set_


# ---- the BGZF route ---------------------------------------------------------------------------------------------------
def bgzf_submit(ing, slot, cs):
    data, members = bgzf_file([bgzf_member(c.deflate + c.tail, c.text, crc=c.crc, isize=c.isize) for c in cs])
    ing.submit_bgzf(slot, data, members, True)
    return ing.wait(slot)


def check_bgzf(cs, what=""):
    from gramtools_amd import Ingest
    cs = [c for c in cs if "bgzf" in c.routes]
    ing = Ingest(max_text_bytes=8 << 20)
    try:
        res = bgzf_submit(ing, 0, cs)
        bad = cs[res.bad_member].name if res.bad_member < len(cs) else None
        assert res.status & ~NOT_FASTQ == 0, f"{what}status {res.status} at member {res.bad_member}: {bad}"
        got = ing.fetch_text(0)
        at = 0
        for i, c in enumerate(cs):
            assert got[at:at + len(c.text)] == c.text, f"{what}member {i}: {c.name}"
            at += len(c.text)
        assert len(got) == at
    finally:
        ing.close()


@pytest.mark.parametrize("group", list(cases.VALID_GROUPS))
def test_bgzf_valid_streams(group):
    check_bgzf(cases.VALID_GROUPS[group])


def test_bgzf_matches_across_the_flushes():
    assert all(len(c.text) % 1024 == 0 for c in cases.STRADDLE)  # every member starts on a 16-byte boundary: p is the decoder's position
    check_bgzf(cases.STRADDLE)


def test_bgzf_random_members():
    check_bgzf(cases.RANDOM(), what=f"seed {cases.RANDOM_SEED}, ")


def test_bgzf_damage_is_reported_never_decoded():
    from gramtools_amd import Ingest
    good = cases.VALID_GROUPS["fused_literals"][0]
    ing = Ingest(max_text_bytes=1 << 20)
    slot = 0
    try:
        for c in cases.INVALID:
            if "bgzf" not in c.routes:
                continue
            ing.reset()
            res = bgzf_submit(ing, slot, [good, c, good])
            assert res.status != 0 and res.status & BAD_MEMBER and res.bad_member == 1, f"{c.name}: status {res.status}, member {res.bad_member}"
            slot ^= 1
    finally:
        ing.close()


# ---- the plain gzip route ---------------------------------------------------------------------------------------------
def gzip_file(cs, piece, min_member):
    """The cases as gzip members in a row, each at least min_member bytes (a comment in its header), so that no piece meets more
    member ends than it can record (GZ_ENDS 16: checked here for every two pieces in a row)."""
    data, ends = bytearray(), []
    for c in cs:
        hdr = padded_header(max(11, min_member - len(c.deflate) - 8))
        data += gzip_member(c.deflate, c.text, header=hdr)
        ends.append(len(data))
    for i in range(0, len(data) // piece + 1):
        assert sum(1 for e in ends if i * piece <= e < (i + 2) * piece) <= 14, "too many member ends for one piece"
    return bytes(data)


def check_gzip(cs, piece, min_member, what="", **kw):
    cs = [c for c in cs if "gzip" in c.routes]
    text = b"".join(c.text for c in cs)
    got, res, ing = decode(gzip_file(cs, piece, min_member), allow=NOT_FASTQ, **kw)
    ing.close()
    if got == text:
        return
    failed = []  # which one: each member on its own
    for i, c in enumerate(cs):
        g1, r1, ing = decode(gzip_member(c.deflate, c.text), allow=NOT_FASTQ)
        ing.close()
        if g1 != c.text:
            failed.append(f"{what}member {i}: {c.name} (status {r1[-1].status})")
    assert not failed, failed
    assert got == text, f"{what}statuses {[r.status for r in res]}; every member decodes on its own"


def test_gzip_small_valid_streams(pieces):
    pieces(1024)
    check_gzip([c for c in cases.VALID if not c.big and c not in cases.STRADDLE], 1024, 160)


def test_gzip_large_valid_streams(pieces):
    pieces(16384)
    check_gzip([c for c in cases.VALID if c.big], 16384, 2400)


def test_gzip_matches_across_the_flushes(pieces):
    pieces(8192)
    check_gzip(cases.STRADDLE, 8192, 1100)


def test_gzip_random_members(pieces):
    """All 300 random block specifications, three to a member (a few blocks each): the members test_deflate_craft_host.py pins to zlib."""
    pieces(4096)
    cs = cases.RANDOM_GZIP()
    assert len(cs) == 100
    check_gzip(cs, 4096, 600, what=f"seed {cases.RANDOM_SEED}, ")


@pytest.mark.parametrize("printable", [True, False])
def test_gzip_references_in_front_of_a_piece(pieces, printable):
    """The first token of a piece's first block is a match into the text in front of the piece (placeholders 256 + j, resolved
    through the 32 KB windows); a byte carried through four pieces; the same across chunk cuts. With printable text the block
    finder can take the starts; with other bytes every later piece is decoded by the link kernel's repair."""
    pieces(cases.FRONT_PIECE)
    data, text, cuts = cases.piece_front_stream(printable)
    for kw in ({}, {"cuts": cuts}, {"cuts": cuts[:1]}):
        got, res, ing = decode(data, allow=NOT_FASTQ, **kw)
        repairs = ing.gzip_repairs()
        ing.close()
        print(f"printable {printable} {kw}: statuses {[r.status for r in res]}, repairs {repairs}")
        assert got is not None, [r.status for r in res]
        assert got == text, next(i for i in range(len(text)) if got[i:i + 1] != text[i:i + 1])
        if not printable:
            assert repairs > 0
        elif not kw:  # one chunk: a finder that took no start would repair every piece behind the stored block (a dozen)
            later = len(data) // cases.FRONT_PIECE - 33
            assert later >= 12 and repairs * 4 <= later, (repairs, later)


def test_gzip_damage_is_reported_never_decoded(pieces):
    pieces(4096)
    for c in cases.INVALID:
        if "gzip" not in c.routes:
            continue
        if c.trunc:  # the file ends there
            data = GZ_HDR + c.deflate
        else:
            data = c.gz_prefix + gzip_member(c.deflate + c.tail, c.text, crc=c.crc, isize=c.isize)
        got, res, ing = decode(data, allow=NOT_FASTQ)
        ing.close()
        want = BAD_CRC if c.isize is not None else BAD_MEMBER  # (a wrong ISIZE is found where the CRC is: gmx_gz_check_kernel)
        assert got is None and res[-1].status != 0 and res[-1].status & want, f"{c.name}: status {res[-1].status}"

"""No GPU: the generator of record_scan_common.py round-trips through the plain-Python parse at the sizes test_record_scan_scale.py
uses, and every one of that test's cases sits exactly on the boundary it is named for — tile counts, scan blocks and lanes, the
2^20-th read inside a plane word, lines / reads / bytes against cap_lines, cap_reads and max_text_bytes. A case that silently
misses its branch fails here."""
import numpy as np
import pytest

import record_scan_common as rs


def _round_trip(kind, g):
    assert rs.parse(kind, g.text) == g.seqs
    assert len(g.starts) == len(g.seqs) + 1 and g.starts[0] == 0 and g.starts[-1] == len(g.text)


@pytest.mark.parametrize("kind,wrap", [("fastq", 0), ("lines", 0), ("fasta", 0), ("fasta", 1), ("fasta", 7), ("fasta", 40)])
def test_generator_round_trips_and_lays_records_out_as_documented(kind, wrap):
    lens = rs.lengths(7, 3000, 1, 40)
    g = rs.generate(kind, lens, 8, wrap=wrap)
    _round_trip(kind, g)
    assert [len(s) for s in g.seqs] == lens.tolist() and set("".join(g.seqs)) == set("ACGT")
    first = {"fastq": b"@", "fasta": b">"}.get(kind)
    for i in (0, 1, 1500, 2999):
        record = g.text[g.starts[i]:g.starts[i + 1]]
        s, n = g.seqs[i].encode(), int(lens[i])
        if kind == "fastq":
            assert record == b"@\n" + s + b"\n+\n" + b"I" * n + b"\n"
        elif kind == "lines":
            assert record == s + b"\n"
        else:
            w = wrap or n
            assert record == b">\n" + b"".join(s[k:k + w] + b"\n" for k in range(0, n, w))
        assert first is None or record[:1] == first


def test_tile_scan_files_reach_the_second_level():
    one = rs.tile_file()
    _round_trip("fastq", one)
    assert 3 << 20 < len(one.text) <= rs.TILE_MAX_TEXT
    assert rs.n_tiles(len(one.text)) == rs.SCAN_BLOCK + 1  # tile_blk[1] holds one tile's newlines
    two = rs.tile_file_two_chunks()
    _round_trip("fastq", two)
    cut = rs.TILE_FIRST_CUT
    assert cut not in two.starts and len(two.text) - cut <= rs.TILE_MAX_TEXT
    assert rs.n_tiles(len(two.text) - cut) > 2 * rs.SCAN_BLOCK  # tile_blk[2]
    assert int(np.searchsorted(two.starts, cut)) > 100          # reads in the first chunk too, and a carried start for the second
    for g in (one, two):
        assert len(g.seqs) <= rs.cap_reads(rs.TILE_MAX_TEXT) and min(map(len, g.seqs)) >= 100 and max(map(len, g.seqs)) <= 150


@pytest.mark.parametrize("n,per,full,rest", [(70000, 2, 34, 1), (65 * 1024 + 1, 2, 33, 0), (129 * 1024 + 5, 3, 43, 1)])
def test_level2_files_give_every_lane_more_than_one_block(n, per, full, rest):
    assert n in rs.LEVEL2_READS
    assert rs.level2_per(rs.scan_blocks(n)) == per and rs.level2_busy_lanes(rs.scan_blocks(n)) == (full, rest)
    for kind in ("fastq", "lines", "fasta"):
        g = rs.level2_file(kind, n)
        _round_trip(kind, g)
        assert len(g.text) <= rs.LEVEL2_MAX_TEXT and n <= rs.cap_reads(rs.LEVEL2_MAX_TEXT)
        assert len(set(map(len, g.seqs))) > 1  # ragged: the offsets scans run
        lines = g.text.count(b"\n")
        assert lines <= rs.cap_lines(rs.LEVEL2_MAX_TEXT)
        if kind == "fasta":  # the lines scan goes over more than 64 blocks, and records of several lines cross block edges
            assert rs.level2_per(rs.scan_blocks(lines)) > 1 and max(map(len, g.seqs)) > 7
        if kind == "lines":
            assert rs.level2_per(rs.scan_blocks(lines)) == per
        cut = rs.level2_cut(g)  # the two-chunk form: inside a record, and the first chunk alone still has per > 1
        assert cut not in g.starts and g.text[cut - 1:cut] != b">"
        n_first = int(np.searchsorted(g.starts, cut)) - 1
        assert n_first == n - rs.LEVEL2_CUT_BEFORE_END and rs.level2_per(rs.scan_blocks(n_first)) > 1


def test_million_read_files_put_the_second_launch_inside_a_plane_word():
    for kind in ("fastq", "lines"):
        g = rs.million_file(kind)
        _round_trip(kind, g)
        n = len(g.seqs)
        assert n == rs.SUB + 700 and rs.SUB < n <= rs.cap_reads(rs.MILLION_MAX_TEXT) == rs.SUB + 1024
        assert len(g.text) <= rs.MILLION_MAX_TEXT and g.text.count(b"\n") <= rs.cap_lines(rs.MILLION_MAX_TEXT)
        lens = np.array([len(s) for s in g.seqs])
        assert lens.min() == 5 and lens.max() == 12
        offsets = np.concatenate([[0], np.cumsum(lens)])
        assert int(offsets[rs.SUB]) % 32 != 0  # the launch of reads 2^20.. starts inside a plane word
        sub = rs.expected_sub_pairs(offsets, n)
        assert sub[0] == 0 and sub[1] == (int(offsets[rs.SUB]) >> 5) + rs.SUB and sub[2:] == [0] * 14
        if kind == "fastq":
            assert int(np.diff(g.starts).max()) < 32  # records under 32 bytes: what lets 2^20 of them into 32 MiB
    assert rs.million_file("fastq").seqs == rs.million_file("lines").seqs


def test_uniform_million_read_file():
    g = rs.uniform_file()
    _round_trip("lines", g)
    assert len(g.seqs) == rs.SUB + 700 and set(map(len, g.seqs)) == {33}
    assert rs.MILLION_MAX_TEXT < len(g.text) <= rs.UNIFORM_MAX_TEXT and len(g.seqs) <= rs.cap_reads(rs.UNIFORM_MAX_TEXT)
    assert rs.expected_sub_pairs(None, len(g.seqs), 33) == [i * 2 * rs.SUB for i in range(16)]


def test_capacity_cases_sit_on_their_boundaries():
    cr, cl = rs.cap_reads(rs.CAP_MAX_TEXT), rs.cap_lines(rs.CAP_MAX_TEXT)
    assert (cr, cl) == (3072, 12296)
    cases = {c.name: c for c in rs.capacity_cases()}
    assert len(cases) == 11
    seen = set()
    for c in cases.values():
        assert len(c.text) <= rs.CAP_MAX_TEXT, c.name
        newlines = c.text.count(b"\n")
        lines = newlines + (0 if c.text.endswith(b"\n") else 1)
        reads = rs.parse(c.kind, c.text)
        heads = len(reads)
        n = heads - 1 if c.kind == "fasta" and not c.final else heads
        if c.fits:
            assert reads[:n] == c.seqs and len(c.seqs) == n
        if c.site == "tile":  # the newline count decides, in front of everything else
            assert newlines == (cl if c.fits else cl + 1) and n == cr, c.name
        else:                 # ... else it passes, and the read count decides
            assert newlines <= cl and n == (cr if c.fits else cr + 1), c.name
        if c.kind == "fastq":
            assert lines == newlines == 4 * heads and c.final
        if c.kind == "fasta":
            assert c.carried == (0 if c.final else len(c.text) - c.text.rindex(b">")) and c.text.endswith(b"\n")
        if c.name.endswith("open-line"):
            assert (newlines, lines, n) == (cl, cl + 1, cr)
        seen.add((c.kind, c.site, c.final, c.fits))
    assert seen == {("fastq", "records", True, True), ("fastq", "records", True, False), ("lines", "lines2", True, True), ("lines", "lines2", True, False),
                    ("lines", "tile", True, True), ("lines", "tile", True, False), ("fasta", "lines2", False, True), ("fasta", "lines2", False, False),
                    ("fasta", "lines2", True, True), ("fasta", "lines2", True, False)}
    for kind in ("fastq", "lines", "fasta"):
        _round_trip(kind, rs.small_good_file(kind))


@pytest.mark.parametrize("kind", ["fastq", "lines"])
@pytest.mark.parametrize("cr", [False, True])
def test_edge_sweep_puts_its_bytes_where_it_says(kind, cr):
    starts, ends = set(), set()
    for t in rs.EDGE_TAILS:
        e = rs.edge_chunks(kind, t, cr)
        assert max(len(e.first), t + len(e.second)) <= rs.EDGE_MAX_TEXT
        assert rs.parse(kind, e.first + e.second) == e.seqs_first + e.seqs_second
        # the first chunk: complete records and t bytes of the next, which is longer than a tile and holds no newline before t + 1
        whole = e.first[:len(e.first) - t]
        assert rs.parse(kind, whole) == e.seqs_first and (not whole or whole.endswith(b"\n"))
        if kind == "lines":
            assert b"\n" not in e.first[len(whole):]
        a, b = e.nl_at
        assert a % rs.TILE == rs.TILE - 1 and b % rs.TILE == 0 and e.second[a:a + 1] == b"\n" == e.second[b:b + 1]
        assert not e.second.endswith(b"\n") and e.second.endswith(b"\r") == cr
        assert len(e.second) % 16 == e.end_residue == rs.edge_end_residue(t)
        starts.add((rs.CARRY - t) % 16)
        ends.add(len(e.second) % 16)
    assert starts == set(range(16)) == ends
    assert {(rs.CARRY - t) // rs.TILE for t in (4095, 4096, 4097)} == {rs.CARRY // rs.TILE - 1, rs.CARRY // rs.TILE - 2}

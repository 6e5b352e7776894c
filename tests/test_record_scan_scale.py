"""The device record scan (gmx_ingest_records.h) at its scale edges: the second level of the tile scan (more than 1024 tiles of
text), ing_scan_level2 with more than 64 blocks (the serial loop inside a lane), ragged chunks of more than 2^20 reads
(sub_pairs[1], and the second launch of Quasimapper.map_ingested), the last size that fits cap_reads / cap_lines and the first
that does not, and newlines and text ends at every 16-byte and tile edge as a deterministic sweep.

The reference is never the code under test: the reads are a plain-Python parse of the file's bytes (record_scan_common.parse),
planes / offsets / skip flags the host packer's (test_ingest.check_reads), sub_pairs follows from the offsets, and the mapping is
compared with the byte feed of the same reads. test_record_scan_scale_host.py shows without a GPU that every file used here
reaches the branch it is meant for.

Not covered: ing_scan_level2 with per > 1 in the TILE scan (gmx_tile_scan2_kernel) needs more than 65536 tiles, 256 MB of
text in one chunk; the function is one template, and its serial loop runs here through the offsets and the lines scans. BAM's
own scan (gmx_bam_scan2_kernel, the same template) runs over tiles of 4096 bytes too, not over records: 70 000 one-base records
are 2.8 MB, 684 tiles, one block — it goes above 64 blocks from 256 MB as well (4 MB with the smallest GMX_BAM_TILE) and is left
out; a BAM chunk's offsets go through the gmx_offsets kernels covered here."""
import numpy as np
import pytest

import record_scan_common as rs
from test_ingest import check_reads

pytestmark = pytest.mark.gpu


def _fmt(kind):
    from gramtools_amd import GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_FASTQ, GMX_INGEST_FORMAT_LINES
    return {"fastq": GMX_INGEST_FORMAT_FASTQ, "fasta": GMX_INGEST_FORMAT_FASTA, "lines": GMX_INGEST_FORMAT_LINES}[kind]


def _submit(ing, slot, text, final):
    ing.submit_text(slot, text, final)
    res = ing.wait(slot)
    if res.status == 0:
        assert res.consumed_bytes + res.tail_bytes == res.text_bytes
    return res


def _through_chunks(ing, kind, text, cuts, seqs):
    """The file as text chunks cut at `cuts`, over alternating slots: every chunk through check_reads (offsets in full among it);
    returns the chunks' read counts."""
    ing.set_format(_fmt(kind))
    ing.reset()
    edges = [0, *cuts, len(text)]
    got, carried, counts = 0, 0, []
    for k in range(len(edges) - 1):
        piece = text[edges[k]:edges[k + 1]]
        final = k == len(edges) - 2
        res = _submit(ing, k % 2, piece, final)
        assert res.text_bytes == carried + len(piece)
        n = int(res.n_reads)
        check_reads(ing, k % 2, res, seqs[got:got + n])
        got += n
        carried = int(res.tail_bytes)
        counts.append(n)
    assert got == len(seqs) and carried == 0
    return counts


# ---- 1: the second level of the tile scan -----------------------------------------------------------------------------------
def test_tile_scan_second_level():
    """1025 tiles in one chunk (gmx_nl_mark_kernel reads tile_blk[1]); then more than 2048 in a chunk that starts with the record
    the chunk before cut (tile_blk[2], and the carried bytes in front of tile 256)."""
    from gramtools_amd import Ingest
    ing = Ingest(max_text_bytes=rs.TILE_MAX_TEXT)
    one = rs.tile_file()
    assert rs.n_tiles(len(one.text)) == rs.SCAN_BLOCK + 1
    assert _through_chunks(ing, "fastq", one.text, [], one.seqs) == [len(one.seqs)]
    two = rs.tile_file_two_chunks()
    assert rs.n_tiles(len(two.text) - rs.TILE_FIRST_CUT) > 2 * rs.SCAN_BLOCK
    counts = _through_chunks(ing, "fastq", two.text, [rs.TILE_FIRST_CUT], two.seqs)
    assert counts[0] == int(np.searchsorted(two.starts, rs.TILE_FIRST_CUT)) - 1 and sum(counts) == len(two.seqs)
    ing.close()


# ---- 2: ing_scan_level2 with more than 64 blocks ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rs.LEVEL2_READS)
def test_scan_level2_serial_loop(n):
    """More than 65536 ragged reads: gmx_offsets2_kernel scans 69 / 66 / 130 blocks, two or three per lane, with the last busy lane
    partly filled or not. The same reads as one read per line and as FASTA wrapped at 7 (gmx_seq_lines2_kernel over more than 64
    blocks of lines, records of several lines across the blocks' edges). In one chunk, and cut inside a record near the end."""
    from gramtools_amd import Ingest
    ing = Ingest(max_text_bytes=rs.LEVEL2_MAX_TEXT)
    for kind in ("fastq", "lines", "fasta"):
        g = rs.level2_file(kind, n)
        assert _through_chunks(ing, kind, g.text, [], g.seqs) == [n]
        assert _through_chunks(ing, kind, g.text, [rs.level2_cut(g)], g.seqs) == [n - rs.LEVEL2_CUT_BEFORE_END, rs.LEVEL2_CUT_BEFORE_END]
    ing.close()


# ---- 3: more than 2^20 reads in a chunk ------------------------------------------------------------------------------------
def _scan_million(ing, kind):
    g = rs.million_file(kind)
    ing.set_format(_fmt(kind))
    ing.reset()
    res = _submit(ing, 0, g.text, True)
    check_reads(ing, 0, res, g.seqs)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in g.seqs])])
    assert int(offsets[rs.SUB]) % 32 != 0
    assert list(res.sub_pairs) == rs.expected_sub_pairs(offsets, len(g.seqs))
    assert res.sub_pairs[0] == 0 and res.sub_pairs[1] == (int(offsets[rs.SUB]) >> 5) + rs.SUB
    return g, res, offsets


def test_more_than_a_million_ragged_reads_and_their_second_launch():
    """2^20 + 700 FASTQ reads of 5-12 bases in one chunk: sub_pairs[1] (gmx_offsets3_kernel) is the plane word of read 2^20, which
    starts inside a word; map_ingested makes two launches from it, and coverage and per-read outcomes equal the byte feed's."""
    from gramtools_amd import Index, Ingest, PinnedArray, Quasimapper
    from gramtools_amd.synth import bracket_to_ints, nested_prg
    ing = Ingest(max_text_bytes=rs.MILLION_MAX_TEXT)
    g, res, offsets = _scan_million(ing, "fastq")
    n = len(g.seqs)
    ix = Index(bracket_to_ints(nested_prg(71, n_top=8, max_depth=3)), 5)
    seeds = PinnedArray(n, np.uint32)
    seeds.array[:] = (np.arange(n, dtype=np.uint64) * 2654435761 % (2 ** 32)).astype(np.uint32)
    qm = Quasimapper(ix)
    qm.record_outcomes(True)
    qm.map_ingested(res, seeds)
    cov, outcomes = qm.coverage(), qm.outcomes()
    tab = np.zeros(256, dtype=np.uint8)
    tab[np.frombuffer(b"ACGT", dtype=np.uint8)] = (1, 2, 3, 4)
    flat = tab[np.frombuffer("".join(g.seqs).encode(), dtype=np.uint8)]
    ref = Quasimapper(ix)
    ref.record_outcomes(True)
    ref.map_reads(flat, offsets.astype(np.uint64), seeds.array.copy())
    cov_ref, outcomes_ref = ref.coverage(), ref.outcomes()
    assert outcomes.size == n == outcomes_ref.size
    assert np.bincount(outcomes, minlength=256).tolist() == np.bincount(outcomes_ref, minlength=256).tolist()
    assert (outcomes[rs.SUB:] == outcomes_ref[rs.SUB:]).all() and (outcomes == outcomes_ref).all()
    stats = cov_ref.stats.as_dict()
    assert stats["skipped"] == 0 and stats["exact_mapped"] > 1000 and stats["missing_kmer"] > 1000  # (reads of every outcome: the comparison says something)
    assert cov.stats.as_dict() == stats
    assert cov.allele_sum_coverage == cov_ref.allele_sum_coverage
    assert cov.allele_base_coverage == cov_ref.allele_base_coverage
    assert cov.grouped_allele_counts == cov_ref.grouped_allele_counts
    for q in (qm, ref):
        q.close()
    ing.close()
    seeds.close()
    ix.close()


def test_more_than_a_million_ragged_reads_one_per_line():
    """The same reads through the lines kernels (gmx_seq_lines1-3 over 1025 blocks of lines, 17 per lane)."""
    from gramtools_amd import Ingest
    ing = Ingest(max_text_bytes=rs.MILLION_MAX_TEXT)
    _scan_million(ing, "lines")
    ing.close()


def test_more_than_a_million_reads_of_one_length():
    """The uniform form: 2^20 + 700 reads of 33 bases, one per line — no format puts them into 32 MiB (35.7 MB), so this ingest
    takes 35 MiB. All sixteen sub_pairs are (i << 20) * 2 (gmx_layout_kernel)."""
    from gramtools_amd import Ingest
    g = rs.uniform_file()
    ing = Ingest(max_text_bytes=rs.UNIFORM_MAX_TEXT)
    ing.set_format(_fmt("lines"))
    res = _submit(ing, 0, g.text, True)
    check_reads(ing, 0, res, g.seqs)
    assert res.uniform_len == rs.UNIFORM_LEN and int(res.n_pairs) == 2 * len(g.seqs)
    assert list(res.sub_pairs) == rs.expected_sub_pairs(None, len(g.seqs), rs.UNIFORM_LEN) == [i * 2 * rs.SUB for i in range(16)]
    ing.close()


# ---- 4: the capacities -----------------------------------------------------------------------------------------------------
CASES = rs.capacity_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_capacities(case):
    """cap_reads = 3072 and cap_lines = 12296 on a 64 KiB ingest. The last size that fits gives status 0 and every read (the last
    entries of line_end, rec_line, line_base are written); the first that does not gives GMX_INGEST_TOO_MANY_LINES and nothing else,
    no reads, and leaves the slot fit for the next file."""
    from gramtools_amd import Ingest, GMX_INGEST_TOO_MANY_LINES
    ing = Ingest(max_text_bytes=rs.CAP_MAX_TEXT)
    ing.set_format(_fmt(case.kind))
    res = _submit(ing, 0, case.text, case.final)
    if case.fits:
        check_reads(ing, 0, res, case.seqs)
        assert res.tail_bytes == case.carried
    else:
        assert res.status == GMX_INGEST_TOO_MANY_LINES and res.n_reads == 0
    good = rs.small_good_file(case.kind)
    ing.reset()
    check_reads(ing, 0, _submit(ing, 0, good.text, True), good.seqs)
    ing.close()


# ---- 5: newlines and text ends at every 16-byte and tile edge -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fastq", "lines"])
@pytest.mark.parametrize("cr", [False, True], ids=["open-last-line", "cr-ends-last-line"])
def test_edge_sweep(kind, cr):
    """ing_nl_mask16 masks the first and the last 16 bytes against [lo, hi): lo = ING_CARRY_MAX - tail moves over every residue
    modulo 16 and across a tile's edge with the record the first chunk cut (tail 0..17, 4095..4097); the second chunk has a '\\n'
    at bytes 4095 and 4096 of a tile and ends, without '\\n', at every residue modulo 16."""
    from gramtools_amd import Ingest
    ing = Ingest(max_text_bytes=rs.EDGE_MAX_TEXT)
    ing.set_format(_fmt(kind))
    for t in rs.EDGE_TAILS:
        e = rs.edge_chunks(kind, t, cr)
        ing.reset()
        first = _submit(ing, 0, e.first, False)
        check_reads(ing, 0, first, e.seqs_first)
        assert first.tail_bytes == t and first.text_bytes == len(e.first)
        second = _submit(ing, 1, e.second, True)
        check_reads(ing, 1, second, e.seqs_second)
        assert second.text_bytes == t + len(e.second) and second.tail_bytes == 0
    ing.close()

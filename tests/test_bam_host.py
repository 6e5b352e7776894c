"""`gram`'s host reader of BAM reads files (SeqReader's BAM mode, gram_main.cpp) against the restatement of the rules in
bam_common.py: every generated file through `gram _parse_check`, the base error rate through `gram _read_stats`, and the files
that must end the run — a .bam that is none, .sam, .cram, malformed and truncated records. No GPU is needed.

Before BAM was read, a BAM file was taken for one read per line of binary text: the `slow` lines compared here were garbage and
the refused files gave exit status 0."""
import math

import pytest

from bam_common import (bam_bytes, generated_files, malformed_texts, parse_bam, parse_check_line, record, reverse_complement, stats_reads)
from ingest_formats_common import gram, parse_check_lines
from test_ingest import bgzf

FILES = generated_files()


@pytest.mark.parametrize("name,text", FILES, ids=[f[0] for f in FILES])
def test_parse_check_slow_line_equals_the_rules(tmp_path, name, text):
    """The host reader's reads of every generated file (BGZF members of 3 KB: records and the header span members) are those the
    rules give; the four-line FASTQ parser declines the file."""
    path = tmp_path / "reads.bam"
    path.write_bytes(bgzf(text, block=3000))
    out = gram("_parse_check", str(path), "2")
    assert out.returncode == 0, out.stdout
    lines = parse_check_lines(out)
    assert lines["fast"] == "declined", out.stdout
    assert lines["slow"] == parse_check_line(parse_bam(text)), out.stdout


def test_bam_is_detected_by_content_and_the_eof_marker_may_be_missing(tmp_path):
    text = dict(FILES)["ragged-1-259"]
    want = parse_check_line(parse_bam(text))
    for fname, data in (("reads.txt", bgzf(text)), ("no_eof.bam", bgzf(text, block=3000, eof=False)), ("UPPER.BAM", bgzf(text))):
        path = tmp_path / fname
        path.write_bytes(data)
        out = gram("_parse_check", str(path), "1")
        assert out.returncode == 0 and parse_check_lines(out)["slow"] == want, (fname, out.stdout)


def _read_stats(path):
    out = gram("_read_stats", str(path))
    assert out.returncode == 0, out.stdout
    return {k: float(v) for k, v in (f.split("=") for f in out.stdout.split())}


def test_base_error_rate(tmp_path):
    """compute_base_error_rate over a BAM: qualities are 33 + q in sequencing order on both strands (the mean does not depend on
    the order; the read lengths and counts do on every record being read); a file without qualities counts -1 a base, as the
    reference does with the 0xFF bytes; records without bases have no qualities."""
    reads = stats_reads()
    recs = [record(s if i % 2 == 0 else reverse_complement(s), flag=0 if i % 2 == 0 else 0x10, name=f"s{i}", qual=q if i % 2 == 0 else q[::-1])
            for i, (s, q) in enumerate(reads)]
    recs.insert(7, record("", name="empty"))
    text = bam_bytes(recs, [("chr1", 1000)])
    parsed, quals = parse_bam(text, with_quals=True)
    assert [p for p in parsed if p] == [s for s, _ in reads]  # (the writer and the rules agree on what a reverse-strand record holds)
    assert [q for q in quals if q] == [bytes(33 + v for v in q) for _, q in reads]
    (tmp_path / "q.bam").write_bytes(bgzf(text, block=3000))
    got = _read_stats(tmp_path / "q.bam")
    n_bases = sum(len(s) for s, _ in reads)
    mean_q = sum(sum(q) for _, q in reads) / n_bases
    assert got["num_bases"] == n_bases and got["max_read_len"] == max(len(s) for s, _ in reads) and got["no_qual_reads"] == 1
    assert math.isclose(got["mean_pb_error"], 10 ** (-mean_q / 10), rel_tol=1e-4)
    # the same reads as FASTQ: the same numbers
    fq = "".join(f"@s{i}\n{s}\n+\n{''.join(chr(33 + v) for v in q)}\n" for i, (s, q) in enumerate(reads)).encode()
    (tmp_path / "q.fq").write_bytes(fq)
    ref = _read_stats(tmp_path / "q.fq")
    assert (got["num_bases"], got["max_read_len"]) == (ref["num_bases"], ref["max_read_len"])
    assert math.isclose(got["mean_pb_error"], ref["mean_pb_error"], rel_tol=1e-6)
    # absent qualities: every byte 0xFF -> byte 32 -> -1 a base
    text = bam_bytes([record(s, flag=0x10 * (i % 2), name=f"s{i}", qual=None) for i, (s, _) in enumerate(reads)], [("chr1", 1000)])
    (tmp_path / "noq.bam").write_bytes(bgzf(text))
    got = _read_stats(tmp_path / "noq.bam")
    assert got["num_bases"] == n_bases and got["no_qual_reads"] == 0
    assert math.isclose(got["mean_pb_error"], 10 ** 0.1, rel_tol=1e-6)


@pytest.mark.parametrize("fname,data,words", [
    ("reads.bam", b"ACGT\nGGCC\n", ("not BAM",)),
    ("reads.BAM", bgzf(b"@r\nACGT\n+\nIIII\n"), ("not BAM",)),
    ("reads.sam", b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n", ("not supported", "samtools view -b", "samtools fastq")),
    ("reads.cram", b"CRAM\3\0" + bytes(40), ("not supported", "samtools view -b", "samtools fastq")),
], ids=["bam-of-text", "bam-of-bgzf-fastq", "sam", "cram"])
def test_files_that_are_refused(tmp_path, fname, data, words):
    path = tmp_path / fname
    path.write_bytes(data)
    for args in (("_parse_check", str(path), "1"), ("_read_stats", str(path))):
        out = gram(*args)
        assert out.returncode == 1, out.stdout
        assert fname in out.stdout and all(w in out.stdout for w in words), out.stdout


MALFORMED = malformed_texts()


@pytest.mark.parametrize("kind,text,index", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_a_malformed_or_truncated_record_ends_the_run(tmp_path, kind, text, index):
    """The reference takes such a record for the end of the file; here the run ends with exit status 1 and the record's index."""
    from bam_common import BamFormatError
    with pytest.raises(BamFormatError) as e:
        parse_bam(text)
    assert e.value.index == index
    path = tmp_path / "bad.bam"
    path.write_bytes(bgzf(text, block=3000))
    out = gram("_parse_check", str(path), "1")
    assert out.returncode == 1, out.stdout
    assert f"BAM record {index} " in out.stdout and ("malformed" in out.stdout or "truncated" in out.stdout), out.stdout
    assert "slow" not in out.stdout


def test_a_truncated_header_ends_the_run(tmp_path):
    text = dict(FILES)["header-of-700-references"]
    path = tmp_path / "cut.bam"
    path.write_bytes(bgzf(text[:5000], block=3000))
    out = gram("_parse_check", str(path), "1")
    assert out.returncode == 1 and "truncated BAM header" in out.stdout, out.stdout

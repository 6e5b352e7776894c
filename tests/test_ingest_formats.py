"""FASTA and one-read-per-line reads files scanned on the device (include/gmx.h gmx_ingest_set_format; gmx_ingest.hip
gmx_seq_lines1-3 / gmx_seq_records / gmx_seq_pack): checked against a restatement of the formats' rules in Python
(ingest_formats_common.py, pinned to `gram`'s host reader by test_ingest_formats_host.py) packed by the host packer, and end to
end through `gram` against the host reader and the same reads as four-line FASTQ."""
import gzip
import json

import numpy as np
import pytest

from bam_common import bam_bytes, header_length, record, reverse_complement
from ingest_formats_common import cli_reads, fasta_text, generated_files, gram, parse, parse_check_lines
from test_ingest import bgzf, check_reads, expected_planes

pytestmark = pytest.mark.gpu

FILES = generated_files()


def _fmt(kind):
    from gramtools_amd import GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_LINES
    return GMX_INGEST_FORMAT_FASTA if kind == "fasta" else GMX_INGEST_FORMAT_LINES


def _check_chunk(ing, slot, res, seqs, got):
    """One chunk's result against the next reads of the file; returns how many it held."""
    assert res.status == 0, f"status {res.status}"
    n = int(res.n_reads)
    assert got + n <= len(seqs)
    if n:
        check_reads(ing, slot, res, seqs[got:got + n])
    else:
        assert res.n_bases == 0 and res.n_pairs == 0
    return n


def _through_text_chunks(ing, data, chunk, seqs):
    ing.reset()
    got, bases, slot, carried = 0, 0, 0, 0
    cuts = list(range(0, len(data), chunk)) or [0]
    for k, at in enumerate(cuts):
        final = k == len(cuts) - 1
        ing.submit_text(slot, data[at:at + chunk], final)
        res = ing.wait(slot)
        got += _check_chunk(ing, slot, res, seqs, got)
        bases += int(res.n_bases)
        assert res.text_bytes == carried + len(data[at:at + chunk])  # (the carried start of the chunk's first record included)
        assert res.consumed_bytes + res.tail_bytes == res.text_bytes
        carried = int(res.tail_bytes)
        if final:
            assert res.tail_bytes == 0
        slot ^= 1
    assert got == len(seqs) and bases == sum(len(s) for s in seqs)


@pytest.mark.parametrize("name,kind,data", FILES, ids=[f[0] for f in FILES])
def test_text_chunks(name, kind, data):
    """Every generated file in ONE chunk and cut into chunks of 64, 333 and 777 bytes over alternating slots (cuts inside headers,
    inside sequence lines, between '\\r' and '\\n', in front of a '>'): read counts, bases, uniform_len, offsets, skip flags and
    planes of every chunk equal the host packer's of the reads the rules give."""
    from gramtools_amd import Ingest
    seqs = parse(kind, data)
    ing = Ingest(max_text_bytes=1 << 20)
    ing.set_format(_fmt(kind))
    for chunk in (len(data), 64, 333, 777):
        _through_text_chunks(ing, data, chunk, seqs)
    ing.close()


def test_all_reads_empty_is_a_ragged_chunk():
    """Reads of length 0 only: uniform_len == 0 means "ragged" to every consumer, so the chunk comes with offsets and one (empty)
    pair per read."""
    from gramtools_amd import Ingest, GMX_INGEST_FORMAT_FASTA
    ing = Ingest(max_text_bytes=1 << 16)
    ing.set_format(GMX_INGEST_FORMAT_FASTA)
    ing.submit_text(0, b">a\n>b\n\n>c\n", True)
    res = ing.wait(0)
    assert (res.status, res.n_reads, res.n_bases, res.uniform_len, res.n_pairs) == (0, 3, 0, 0, 3)
    got = ing.fetch_reads(0, res)
    assert got.offsets.tolist() == [0, 0, 0, 0] and not got.planes[:3].any() and not got.skip[:3].any()
    ing.close()


def test_a_header_line_in_a_lines_file_and_sequence_before_a_fasta_header_are_declined():
    from gramtools_amd import Ingest, GMX_INGEST_BAD_RECORD, GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_LINES
    ing = Ingest(max_text_bytes=1 << 16)
    ing.set_format(GMX_INGEST_FORMAT_LINES)
    for k, text in enumerate((b"ACGT\nGGCC\n>x\nACGT\n", b"ACGT\n@x\nACGT\n")):
        ing.reset()
        ing.submit_text(k, text, True)
        assert ing.wait(k).status == GMX_INGEST_BAD_RECORD
    ing.set_format(GMX_INGEST_FORMAT_FASTA)
    ing.reset()
    ing.submit_text(0, b"\nACGT\n>x\nACGT\n", True)
    assert ing.wait(0).status == GMX_INGEST_BAD_RECORD
    ing.close()


def _one_list_of_reads(variant):
    """Lengths at the edges of a plane word (32 bases) and, ragged, of the offsets form: the reads follow each other at every kind
    of offset modulo 32, so (off + len) >> 5 crosses no word, one and several."""
    rng = np.random.default_rng(11)
    seq = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    if variant == "uniform":
        return [seq(33) for _ in range(40)]
    lens = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 7, 8, 16, 45, 50]
    seqs = [seq(n) for n in lens + lens[::-1] + [64, 32, 32, 1, 31, 97, 2, 96]]
    if variant == "unencodable":  # an unencodable base at positions 0, 31, 32 and len - 1, in reads next to clean ones
        for r, at in ((0, 0), (3, 31), (4, 32), (6, 31), (7, 32), (9, 0), (10, 96), (12, 7), (14, 31), (21, 32), (25, 63)):
            assert at < len(seqs[r])
            seqs[r] = seqs[r][:at] + "N" + seqs[r][at + 1:]
    return seqs


def _five_ways(seqs):
    """(name, format, text, BAM header bytes) of the same reads; the BAM stores every second read on the reverse strand."""
    from gramtools_amd import GMX_INGEST_FORMAT_BAM, GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_FASTQ, GMX_INGEST_FORMAT_LINES
    bam = bam_bytes([record(reverse_complement(s) if i % 2 else s, flag=0x10 if i % 2 else 0, name=f"r{i}") for i, s in enumerate(seqs)], [("chr1", 1000)])
    return [("fastq", GMX_INGEST_FORMAT_FASTQ, "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(seqs)).encode(), 0),
            ("fasta-wrap7", GMX_INGEST_FORMAT_FASTA, fasta_text(seqs, 7), 0),
            ("fasta", GMX_INGEST_FORMAT_FASTA, fasta_text(seqs), 0),
            ("lines", GMX_INGEST_FORMAT_LINES, "".join(s + "\n" for s in seqs).encode(), 0),
            ("bam", GMX_INGEST_FORMAT_BAM, bam, header_length(bam))]


@pytest.mark.parametrize("variant", ["ragged", "uniform", "unencodable"])
def test_the_same_reads_in_every_format_give_the_same_planes(variant):
    """One list of reads as four-line FASTQ, FASTA wrapped at 7 (the gather across lines), FASTA unwrapped, one read per line and
    BAM with every second record on the reverse strand (odd and even mirrored window starts), each in one chunk: the pack kernels
    place a read's words by one rule (ing_pack_words; gmx_bam_pack_kernel has it written out), so planes, offsets and skip flags
    are bit-identical across the formats and equal the host packer's. With unencodable bases ('N'; BAM code 15) the skip flags agree, any_skip is set and the other reads' planes
    are untouched (a flagged read's own planes are whatever its letters' bits give: they are not compared)."""
    from gramtools_amd import Ingest
    seqs = _one_list_of_reads(variant)
    exp, offs, uniform = expected_planes(seqs)
    assert uniform == (33 if variant == "uniform" else 0)
    skip_exp = np.array([0 if set(s) <= set("ACGT") else 1 for s in seqs], dtype=np.uint8)
    assert bool(skip_exp.any()) == (variant == "unencodable")
    keep = np.ones(int(exp.planes.size), dtype=bool)  # the pairs of the reads without an unencodable base, and the ragged form's spare ones
    for r in np.flatnonzero(skip_exp):
        p0 = (int(offs[r]) >> 5) + int(r)
        keep[p0:p0 + (len(seqs[r]) + 31) // 32] = False
    ing = Ingest(max_text_bytes=1 << 16)
    first = None
    for name, fmt, text, header in _five_ways(seqs):
        ing.set_format(fmt)
        ing.reset()
        if header:
            ing.set_bam_header(header)
        ing.submit_text(0, text, True)
        res = ing.wait(0)
        assert (res.status, res.n_reads, res.uniform_len, res.n_bases) == (0, len(seqs), uniform, int(offs[-1])), name
        assert bool(res.any_skip) == bool(skip_exp.any()), name
        n_pairs = int(res.n_pairs)
        assert n_pairs == (len(seqs) * 2 if uniform else (int(offs[-1]) >> 5) + len(seqs)), name
        got = ing.fetch_reads(0, res)
        planes = np.where(keep[:n_pairs], got.planes[:n_pairs], 0)
        assert (planes == np.where(keep[:n_pairs], exp.planes[:n_pairs], 0)).all(), name  # (b) the host packer's
        assert (got.skip[:len(seqs)] == skip_exp).all(), name
        assert uniform or (got.offsets == offs).all(), name
        if first is None:
            first = (planes, got.skip.copy(), got.offsets)
        else:  # (a) bit-identical across the formats
            assert (planes == first[0]).all() and (got.skip == first[1]).all(), name
            assert uniform or (got.offsets == first[2]).all(), name
    ing.close()


def _container_file():
    rng = np.random.default_rng(5)
    seqs = ["".join("ACGTN"[int(x)] for x in rng.integers(0, 5 if i % 13 == 0 else 4, size=int(rng.integers(1, 260)))) for i in range(3000)]
    return fasta_text(seqs, 60), seqs


def test_bgzf_container():
    """A ragged wrapped FASTA as BGZF, members of 3 KB in chunks of five: records span members and chunks."""
    from gramtools_amd import Ingest, bgzf_members, GMX_INGEST_FORMAT_FASTA
    text, seqs = _container_file()
    data = bgzf(text, block=3001)
    mem = bgzf_members(data)
    ing = Ingest(max_text_bytes=1 << 20)
    ing.set_format(GMX_INGEST_FORMAT_FASTA)
    chunks = [mem[i:i + 5] for i in range(0, len(mem), 5)]
    got, slot = 0, 0
    for ci, ch in enumerate(chunks):
        lo, hi = ch[0][0], ch[-1][0] + ch[-1][1]
        ing.submit_bgzf(slot, data[lo:hi], [(o - lo, s, i, c) for o, s, i, c in ch], ci == len(chunks) - 1)
        got += _check_chunk(ing, slot, ing.wait(slot), seqs, got)
        slot = (slot + 1) % 3
    assert got == len(seqs)
    ing.close()


def test_gzip_container(monkeypatch):
    """The same file as plain gzip: chunks of a few pieces of 2 KB."""
    from gramtools_amd import Ingest, GMX_INGEST_FORMAT_FASTA
    monkeypatch.setenv("GMX_GZ_PIECE", "2048")
    text, seqs = _container_file()
    data = gzip.compress(text, 6)
    ing = Ingest(max_text_bytes=4 << 20)
    ing.set_format(GMX_INGEST_FORMAT_FASTA)
    chunk, look, got, n = 7000, 1 << 18, 0, len(data)
    for k, at in enumerate(range(0, n, chunk)):
        end = min(n, at + chunk)
        final = end == n
        ing.submit_gzip(k % 2, data[at:end if final else min(n, end + look)], end - at, final)
        got += _check_chunk(ing, k % 2, ing.wait(k % 2), seqs, got)
    assert got == len(seqs)
    ing.close()


def test_chunks_dealt_over_two_ingests():
    """submit_text_deferred / scan / fetch_tail: the record a chunk's end cuts (from its last header on) travels through the host."""
    from gramtools_amd import Ingest, GMX_INGEST_FORMAT_FASTA
    text, seqs = _container_file()
    ings = [Ingest(max_text_bytes=1 << 20) for _ in range(2)]
    for ing in ings:
        ing.set_format(GMX_INGEST_FORMAT_FASTA)
    chunk = 5003
    cuts = list(range(0, len(text), chunk))
    submit = lambda c: ings[c % 2].submit_text_deferred((c // 2) & 1, text[cuts[c]:cuts[c] + chunk])  # noqa: E731
    for c in range(min(len(cuts), 4)):
        submit(c)
    got, tail = 0, b""
    for c in range(len(cuts)):
        ing, slot = ings[c % 2], (c // 2) & 1
        ing.scan(slot, tail, c == len(cuts) - 1)
        res = ing.wait(slot)
        got += _check_chunk(ing, slot, res, seqs, got)
        tail = ing.fetch_tail(slot)
        assert len(tail) == res.tail_bytes
        if c + 4 < len(cuts):
            submit(c + 4)
    assert got == len(seqs) and tail == b""
    for ing in ings:
        ing.close()


def test_default_format_is_untouched():
    """Without set_format a FASTA is still GMX_INGEST_BAD_RECORD; an unknown format and a format set under a chunk in flight are
    GMX_EINVAL; back on FASTQ the same ingest reads four-line FASTQ as before."""
    from gramtools_amd import Ingest, GmxError, GMX_INGEST_BAD_RECORD, GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_FASTQ
    from test_ingest import fastq
    text, seqs = _container_file()
    text, seqs = text[:200000], None
    ing = Ingest(max_text_bytes=1 << 20)
    ing.submit_text(0, text, True)
    assert ing.wait(0).status & GMX_INGEST_BAD_RECORD
    with pytest.raises(GmxError) as e:
        ing.set_format(7)
    assert e.value.code == -1
    fq_text, fq_seqs = fastq(np.random.default_rng(2), 2000, 40, 160, bad_every=9)
    ing.reset()
    ing.submit_text(1, fq_text, True)
    with pytest.raises(GmxError) as e:  # a chunk in flight
        ing.set_format(GMX_INGEST_FORMAT_FASTA)
    assert e.value.code == -1
    check_reads(ing, 1, ing.wait(1), fq_seqs)
    ing.set_format(GMX_INGEST_FORMAT_FASTA)
    ing.reset()
    ing.submit_text(0, text, False)
    res = ing.wait(0)
    assert res.status == 0 and res.n_reads > 0
    ing.set_format(GMX_INGEST_FORMAT_FASTQ)
    ing.reset()
    ing.submit_text(1, fq_text, True)
    check_reads(ing, 1, ing.wait(1), fq_seqs)
    ing.close()


def _reads_file(kind, seqs):
    return fasta_text(seqs, 60) if kind == "fasta" else "".join(s + "\n" for s in seqs).encode()


@pytest.mark.parametrize("kind", ["fasta", "lines"])
@pytest.mark.parametrize("container,chunk", [("plain", "100000000"), ("plain", "333"), ("gz", "100000000"), ("bgzf", "100000000"), ("bgzf", "333")])
def test_gram_parse_check_device_line(tmp_path, kind, container, chunk):
    """`gram _parse_check` with GMX_PARSE_CHECK_DEVICE=any: the format is detected and set as `gram genotype` does, and the device
    line equals the general reader's. (GMX_TEXT_CHUNK for plain text; BGZF members of 3 KB in chunks of two for "333".)"""
    data = _reads_file(kind, cli_reads(2500, 31))
    path = tmp_path / ("r." + ("fa" if kind == "fasta" else "txt") + ("" if container == "plain" else ".gz"))
    path.write_bytes(data if container == "plain" else gzip.compress(data, 6) if container == "gz" else bgzf(data, block=3000))
    env = {"GMX_PARSE_CHECK_DEVICE": "any", "GMX_TEXT_CHUNK": chunk, "GMX_GZ_PIECE": "2048"}
    if chunk == "333":
        env["GMX_INGEST_MEMBERS"] = "2"
    out = gram("_parse_check", str(path), "2", env=env)
    assert out.returncode == 0, out.stdout
    lines = parse_check_lines(out)
    assert lines["fast"] == "declined" and lines["device"] == lines["slow"], out.stdout
    assert lines["slow"].split()[0] == "2500"


@pytest.mark.parametrize("kind", ["fasta", "lines"])
def test_gram_genotype_on_the_device_equals_the_host_reader(tmp_path, kind):
    """`gram genotype` on two reads files (the 5000-draw seeding carries across them) of ragged reads with Ns, written as wrapped
    FASTA / one read per line: the device route (default) in one chunk, in small chunks, as .gz, as BGZF, over two engines and with
    the host reader taking over in the middle of the first file — against the host reader forced and the same reads as four-line
    FASTQ: the three coverage files, the five counters and the read depth are byte-identical."""
    from gramtools_amd.synth import random_ref, snp_prg, simulate_snp_reads
    rng = np.random.default_rng(3)
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    (tmp_path / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    reads = simulate_snp_reads(ref, pos, alts, n_alts, 7300, 60, 6)
    txt = ["".join("ACGT"[b - 1] for b in r) for r in reads]
    txt = [t[:int(rng.integers(20, 61))] for t in txt]  # ragged
    for i in range(0, len(txt), 97):
        txt[i] = txt[i][:7] + "N" + txt[i][8:]
    fq = lambda rs: "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(rs)).encode()  # noqa: E731
    wr = lambda rs: fasta_text(rs, 25) if kind == "fasta" else "".join(s + "\n" for s in rs).encode()  # noqa: E731
    for tag, rs in (("a", txt[:5100]), ("b", txt[5100:])):
        (tmp_path / f"{tag}.fq").write_bytes(fq(rs))
        (tmp_path / f"{tag}.seq").write_bytes(wr(rs))
        (tmp_path / f"{tag}.seq.gz").write_bytes(gzip.compress(wr(rs), 6))
        (tmp_path / f"{tag}.seq.bgz").write_bytes(bgzf(wr(rs), block=9000))
    runs = (("fastq", ("a.fq", "b.fq"), {"GMX_HOST_FASTQ": "1"}),
            ("host", ("a.seq", "b.seq"), {"GMX_HOST_FASTQ": "1", "GMX_HOST_GZ": "1"}),
            ("device", ("a.seq", "b.seq"), {}),
            ("device-777", ("a.seq", "b.seq"), {"GMX_TEXT_CHUNK": "777"}),
            ("gz", ("a.seq.gz", "b.seq.gz"), {"GMX_GZ_CHUNK": "20000", "GMX_GZ_PIECE": "4096"}),
            ("bgzf", ("a.seq.bgz", "b.seq.bgz"), {"GMX_INGEST_MEMBERS": "3"}),
            ("two-engines", ("a.seq", "b.seq.bgz"), {"DEVICES": "0,0", "GMX_TEXT_CHUNK": "1000", "GMX_INGEST_MEMBERS": "2"}),
            ("takeover", ("a.seq", "b.seq"), {"GMX_TEXT_CHUNK": "30000", "GMX_INGEST_TEST_FAIL_CHUNK": "2"}),
            ("takeover-bgzf", ("a.seq.bgz", "b.seq"), {"GMX_INGEST_MEMBERS": "3", "GMX_INGEST_TEST_FAIL_CHUNK": "2"}))
    outs = {}
    for name, files, env in runs:
        env = dict(env, GMX_FEED_TRACE="1")
        out = tmp_path / name
        extra = ["--devices", env.pop("DEVICES")] if "DEVICES" in env else []
        r = gram("genotype", "--gram_dir", str(tmp_path), "--reads", *[str(tmp_path / f) for f in files], "--sample_id", "s", "--ploidy", "diploid",
                 "--kmer_size", "6", "--genotype_dir", str(out), "--seed", "1234", *extra, env=env)
        assert r.returncode == 0, (name, r.stdout)
        if name.startswith("takeover"):
            assert "gave up after" in r.stdout and "the host reader takes over" in r.stdout, r.stdout
            assert "gave up after 0 reads" not in r.stdout, r.stdout
        if name in ("device", "device-777", "takeover"):  # (the route really taken: the feed's trace names its chunks)
            assert "text chunk scanned and packed" in r.stdout, r.stdout
        if name == "host":
            assert "chunk scanned" not in r.stdout and "chunk decoded" not in r.stdout and "chunk submitted" not in r.stdout, r.stdout
        counters = [l for l in r.stdout.splitlines() if l.startswith("Count ")]
        assert len(counters) == 5, r.stdout
        outs[name] = ([(out / "coverage" / f).read_bytes() for f in ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")],
                      counters, json.loads((out / "read_stats.json").read_text())["Read_depth"])
    for name, _, _ in runs[1:]:
        assert outs[name] == outs["fastq"], name

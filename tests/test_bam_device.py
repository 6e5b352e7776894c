"""BAM reads files on the device (include/gmx.h GMX_INGEST_FORMAT_BAM; gmx_ingest.hip gmx_bam_chain / _link / _records / _pack):
every generated file of bam_common.py as text cut at any byte and as BGZF, against the restatement of the rules packed by the
host packer; crafted speculation traps; malformed records and damaged members; the calls that are refused in this format; and
end to end through `gram` against the host reader and the same reads as four-line FASTQ."""
import json

import numpy as np
import pytest

from bam_common import (bam_bytes, generated_files, header_length, malformed_texts, parse_bam, record, reverse_complement, trap_records)
from ingest_formats_common import gram, parse_check_lines
from test_ingest import bgzf, check_reads

pytestmark = pytest.mark.gpu

FILES = generated_files()


def _bam_ingest(max_text=1 << 20):
    from gramtools_amd import Ingest, GMX_INGEST_FORMAT_BAM
    ing = Ingest(max_text_bytes=max_text)
    ing.set_format(GMX_INGEST_FORMAT_BAM)
    return ing


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
    ing.set_bam_header(header_length(data))
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


def _through_bgzf_chunks(ing, text, seqs, block=3000, per_chunk=5, eof=True):
    from gramtools_amd import bgzf_members
    data = bgzf(text, block=block, eof=eof)
    mem = [m for m in bgzf_members(data) if m[2]]  # (the EOF marker holds nothing)
    ing.reset()
    ing.set_bam_header(header_length(text))
    chunks = [mem[i:i + per_chunk] for i in range(0, len(mem), per_chunk)]
    got, slot = 0, 0
    for ci, ch in enumerate(chunks):
        lo, hi = ch[0][0], ch[-1][0] + ch[-1][1]
        ing.submit_bgzf(slot, data[lo:hi], [(o - lo, s, i, c) for o, s, i, c in ch], ci == len(chunks) - 1)
        got += _check_chunk(ing, slot, ing.wait(slot), seqs, got)
        slot = (slot + 1) % 3
    assert got == len(seqs)


@pytest.mark.parametrize("name,text", FILES, ids=[f[0] for f in FILES])
def test_text_chunks(name, text):
    """Every generated file in ONE chunk and cut into chunks of 64, 333 and 777 bytes over alternating slots (cuts inside the
    header, inside block_size, inside names, between the two bases of a byte): read counts, bases, uniform_len, offsets, skip flags
    and planes of every chunk equal the host packer's of the reads the rules give."""
    seqs = parse_bam(text)
    ing = _bam_ingest()
    for chunk in (len(text), 64, 333, 777):
        _through_text_chunks(ing, text, chunk, seqs)
    ing.close()


@pytest.mark.parametrize("name,text", FILES, ids=[f[0] for f in FILES])
def test_bgzf_container(name, text):
    """The same files as BGZF, members of 3 KB in chunks of five over three slots: header and records span members and chunks."""
    seqs = parse_bam(text)
    ing = _bam_ingest()
    _through_bgzf_chunks(ing, text, seqs)
    ing.close()


def test_missing_eof_marker_is_accepted():
    text = dict(FILES)["ragged-1-259"]
    ing = _bam_ingest()
    _through_bgzf_chunks(ing, text, parse_bam(text), eof=False)
    ing.close()


@pytest.mark.parametrize("tile", ["64", "128", "256", "1000"])
def test_speculation_traps(monkeypatch, tile):
    """Records whose last tag holds complete plausible records, across the starts of small tiles: the reads are those of the
    rules — nothing inside a tag is ever a read — and tiles were walked again, so the trap was sprung. The counter takes only a
    second walk that adds records, so a chunk's end, where the tile behind a cut record is entered again to find nothing, does not
    raise it: it rises in the chunked runs too only because their tiles guess wrong as well."""
    monkeypatch.setenv("GMX_BAM_TILE", tile)
    text = bam_bytes(trap_records(np.random.default_rng(int(tile)), 400), [("chr1", 100000)])
    seqs = parse_bam(text)
    assert len(seqs) == 400
    ing = _bam_ingest()
    assert ing.bam_rewalks() == 0
    _through_text_chunks(ing, text, len(text), seqs)
    sprung = ing.bam_rewalks()
    assert sprung > 0
    _through_text_chunks(ing, text, 5003, seqs)
    _through_bgzf_chunks(ing, text, seqs, block=3000, per_chunk=7)
    assert ing.bam_rewalks() > sprung
    ing.close()


def test_traps_with_the_default_tile():
    text = bam_bytes(trap_records(np.random.default_rng(1), 2000), [("chr1", 100000)])
    ing = _bam_ingest(4 << 20)
    _through_text_chunks(ing, text, len(text), parse_bam(text))
    assert ing.bam_rewalks() > 0
    ing.close()


MALFORMED = malformed_texts()


@pytest.mark.parametrize("kind,text,index", MALFORMED, ids=[m[0] for m in MALFORMED])
@pytest.mark.parametrize("chunk", [0, 333])
def test_a_malformed_record_is_reported(kind, text, index, chunk):
    """Each of the four kinds, in one chunk and in chunks of 333 bytes: GMX_INGEST_BAD_RECORD, and no chunk before it delivered
    more than the records in front of the malformed one."""
    from gramtools_amd import GMX_INGEST_BAD_RECORD
    ing = _bam_ingest()
    ing.reset()
    ing.set_bam_header(header_length(text))
    chunk = chunk or len(text)
    cuts = list(range(0, len(text), chunk))
    got, status = 0, 0
    for k, at in enumerate(cuts):
        ing.submit_text(k % 2, text[at:at + chunk], k == len(cuts) - 1)
        res = ing.wait(k % 2)
        status = res.status
        if status:
            break
        got += int(res.n_reads)
    assert status & GMX_INGEST_BAD_RECORD, status
    assert got <= index
    ing.close()


def test_a_file_that_ends_inside_its_header_is_reported():
    from gramtools_amd import GMX_INGEST_BAD_RECORD
    text = dict(FILES)["header-of-700-references"]
    ing = _bam_ingest()
    ing.reset()
    ing.set_bam_header(header_length(text))
    ing.submit_text(0, text[:3000], False)
    res = ing.wait(0)
    assert (res.status, res.n_reads, res.tail_bytes) == (0, 0, 0)
    ing.submit_text(1, text[3000:5000], True)
    assert ing.wait(1).status & GMX_INGEST_BAD_RECORD
    ing.close()


def test_a_damaged_member_is_reported():
    from gramtools_amd import bgzf_members, GMX_INGEST_BAD_MEMBER, GMX_INGEST_BAD_CRC
    text = dict(FILES)["ragged-1-259"]
    data = bytearray(bgzf(text, block=3000))
    mem = [m for m in bgzf_members(bytes(data)) if m[2]]
    off, size = mem[3][0], mem[3][1]
    for k in range(off + size // 2, off + size // 2 + 8):
        data[k] ^= 0x5A
    ing = _bam_ingest()
    ing.reset()
    ing.set_bam_header(header_length(text))
    ing.submit_bgzf(0, bytes(data[mem[0][0]:mem[-1][0] + mem[-1][1]]), [(o - mem[0][0], s, i, c) for o, s, i, c in mem], True)
    res = ing.wait(0)
    assert res.status & (GMX_INGEST_BAD_MEMBER | GMX_INGEST_BAD_CRC), res.status
    ing.close()


def test_calls_that_are_refused_and_the_way_back_to_fastq():
    """set_bam_header in another format, and submit_gzip / the deferred submits / scan in BAM format, are GMX_EINVAL; after
    switching back to FASTQ the same ingest reads FASTQ as before."""
    from gramtools_amd import Ingest, GmxError, GMX_INGEST_FORMAT_BAM, GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_FASTQ
    from test_ingest import fastq
    fq_text, fq_seqs = fastq(np.random.default_rng(2), 2000, 40, 160, bad_every=9)
    text = dict(FILES)["ragged-1-259"]
    ing = Ingest(max_text_bytes=1 << 20)

    def refused(call, *args):
        with pytest.raises(GmxError) as e:
            call(*args)
        assert e.value.code == -1

    refused(ing.set_bam_header, 10)  # FASTQ
    ing.set_format(GMX_INGEST_FORMAT_FASTA)
    refused(ing.set_bam_header, 10)
    ing.set_format(GMX_INGEST_FORMAT_FASTQ)
    ing.submit_text(0, fq_text, True)
    check_reads(ing, 0, ing.wait(0), fq_seqs)
    ing.set_format(GMX_INGEST_FORMAT_BAM)
    ing.reset()
    refused(ing.submit_gzip, 0, b"\x1f\x8b" + bytes(30), 32, True)
    refused(ing.submit_text_deferred, 0, text[:100])
    refused(ing.submit_bgzf_deferred, 0, bgzf(text), [])
    refused(ing.scan, 0, b"", True)
    _through_text_chunks(ing, text, 4000, parse_bam(text))
    ing.reset()
    ing.set_bam_header(header_length(text))
    ing.submit_text(0, text[:5000], False)
    refused(ing.set_bam_header, header_length(text))  # a chunk in flight
    assert ing.wait(0).status == 0
    ing.set_format(GMX_INGEST_FORMAT_FASTQ)
    ing.reset()
    ing.submit_text(1, fq_text, True)
    check_reads(ing, 1, ing.wait(1), fq_seqs)
    ing.close()


@pytest.mark.parametrize("name", ["ragged-1-259", "n-equals-iupac", "header-of-700-references", "one-read-of-300k", "header-only", "tag-traps"])
@pytest.mark.parametrize("members", ["7168", "2"])
def test_gram_parse_check_device_line(tmp_path, name, members):
    """`gram _parse_check` with GMX_PARSE_CHECK_DEVICE=any: the file is detected as BAM, its header measured and skipped as `gram
    genotype` does; the device line equals the host reader's, for the whole file at once and for chunks of two 3 KB members."""
    text = dict(FILES)[name]
    path = tmp_path / "reads.bam"
    path.write_bytes(bgzf(text, block=3000))
    out = gram("_parse_check", str(path), "2", env={"GMX_PARSE_CHECK_DEVICE": "any", "GMX_INGEST_MEMBERS": members})
    assert out.returncode == 0, out.stdout
    lines = parse_check_lines(out)
    assert lines["fast"] == "declined" and lines["device"] == lines["slow"], out.stdout
    assert lines["slow"].split()[0] == str(len(parse_bam(text)))


def test_gram_genotype_on_the_device_equals_the_host_reader(tmp_path):
    """`gram genotype` on two reads files (the 5000-draw seeding carries across them) of ragged reads with Ns written as BAM, about
    30 % of the records on the reverse strand (the stored sequence reverse-complemented, flag 0x10: the read recovered is the
    FASTQ's): the device route (default), small chunks, the host reader forced, two engines, and the host reader taking over in
    the middle of the first file — against the same reads as four-line FASTQ: the three coverage files, the five counters and the
    read depth are byte-identical."""
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

    def bam(rs):
        recs = []
        for i, s in enumerate(rs):
            back = rng.random() < 0.3
            recs.append(record(reverse_complement(s) if back else s, flag=(0x10 if back else 0) | (0x4 if i % 5 == 0 else 0), name=f"r{i}", qual=bytes([40]) * len(s)))
        text = bam_bytes(recs, [("chr1", 3000)], "@HD\tVN:1.6\n")
        assert parse_bam(text) == rs
        return bgzf(text, block=9000)

    for tag, rs in (("a", txt[:5100]), ("b", txt[5100:])):
        (tmp_path / f"{tag}.fq").write_bytes(fq(rs))
        (tmp_path / f"{tag}.bam").write_bytes(bam(rs))
    runs = (("fastq", ("a.fq", "b.fq"), {"GMX_HOST_FASTQ": "1"}),
            ("device", ("a.bam", "b.bam"), {}),
            ("device-small-chunks", ("a.bam", "b.bam"), {"GMX_INGEST_MEMBERS": "3"}),
            ("device-16-threads", ("a.bam", "b.bam"), {"THREADS": "16"}),
            ("host", ("a.bam", "b.bam"), {"GMX_HOST_GZ": "1"}),
            ("two-engines", ("a.bam", "b.bam"), {"DEVICES": "0,0", "GMX_INGEST_MEMBERS": "2"}),
            ("takeover", ("a.bam", "b.bam"), {"GMX_INGEST_MEMBERS": "3", "GMX_INGEST_TEST_FAIL_CHUNK": "2"}))
    outs = {}
    for name, files, env in runs:
        env = dict(env, GMX_FEED_TRACE="1")
        out = tmp_path / name
        extra = ["--devices", env.pop("DEVICES")] if "DEVICES" in env else []
        extra += ["--max_threads", env.pop("THREADS")] if "THREADS" in env else []
        r = gram("genotype", "--gram_dir", str(tmp_path), "--reads", *[str(tmp_path / f) for f in files], "--sample_id", "s", "--ploidy", "diploid",
                 "--kmer_size", "6", "--genotype_dir", str(out), "--seed", "1234", *extra, env=env)
        assert r.returncode == 0, (name, r.stdout)
        if name == "takeover":
            assert "gave up after" in r.stdout and "the host reader takes over" in r.stdout, r.stdout
            assert "gave up after 0 reads" not in r.stdout, r.stdout
        if name.startswith("device") or name == "takeover":  # (the route really taken: the feed's trace names its chunks)
            assert "BAM chunk chained and packed" in r.stdout, r.stdout
        if name.startswith("device"):  # (and kept to the end: a chain that gives up after a chunk would still match the FASTQ's output)
            assert "the host reader takes over" not in r.stdout and "gave up after" not in r.stdout, r.stdout
        if name in ("host", "two-engines"):
            assert "chunk chained" not in r.stdout and "chunk decoded" not in r.stdout and "chunk submitted" not in r.stdout, r.stdout
        counters = [l for l in r.stdout.splitlines() if l.startswith("Count ")]
        assert len(counters) == 5, r.stdout
        outs[name] = ([(out / "coverage" / f).read_bytes() for f in ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")],
                      counters, json.loads((out / "read_stats.json").read_text())["Read_depth"])
    for name, _, _ in runs[1:]:
        assert outs[name] == outs["fastq"], name


def test_gram_genotype_refuses_what_it_cannot_read(tmp_path):
    """A .sam, a .cram or a broken BAM given to `gram genotype`: exit status 1 and a message, never an empty result."""
    from gramtools_amd.synth import random_ref, snp_prg
    ref = random_ref(2000, 4)
    prg, _, _, _ = snp_prg(ref, 20, 5)
    (tmp_path / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    (tmp_path / "r.sam").write_bytes(b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n")
    (tmp_path / "r.cram").write_bytes(b"CRAM\3\0" + bytes(40))
    kind, text, index = MALFORMED[0]
    (tmp_path / "broken.bam").write_bytes(bgzf(text, block=3000))
    for fname, words in (("r.sam", ("not supported", "samtools")), ("r.cram", ("not supported", "samtools")), ("broken.bam", (f"BAM record {index} ", "malformed"))):
        r = gram("genotype", "--gram_dir", str(tmp_path), "--reads", str(tmp_path / fname), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", "6",
                 "--genotype_dir", str(tmp_path / ("out_" + fname)), "--seed", "1")
        assert r.returncode == 1, (fname, r.stdout)
        assert all(w in r.stdout for w in words), (fname, r.stdout)

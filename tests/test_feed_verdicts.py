"""What `gram genotype` makes of a chunk the device feed does not take (gram_device_feed.h: the chunk verdict): the fatal
"irregular FASTQ record after the first N reads" behind chunks already mapped, the silent decline where the irregular record
lies in the first chunk, and bytes that are no BGZF member behind chunks already delivered — on one engine and with the chunks
dealt over two. Every record is R bytes long, so the chunk a record lies in, and N, follow from the file alone."""
import numpy as np
import pytest

from test_ingest import _gram, bgzf

pytestmark = pytest.mark.gpu

N_READS, READ_LEN = 3000, 60
R = 9 + (READ_LEN + 1) + 2 + (READ_LEN + 1)  # "@r000017\n" is 9 bytes, then sequence, "+", qualities
C = 5000                                    # bytes of text per chunk: GMX_TEXT_CHUNK, and MEMBERS members of BLOCK bytes
BLOCK, MEMBERS = 2500, 2
COVERAGE_FILES = ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")
TEXT_ENV = {"GMX_TEXT_CHUNK": str(C)}
BGZF_ENV = {"GMX_INGEST_MEMBERS": str(MEMBERS)}


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """The gram directory (a 3 000-base reference, 40 sites) and the reads as text, made once."""
    from gramtools_amd.synth import random_ref, snp_prg, simulate_snp_reads
    root = tmp_path_factory.mktemp("verdicts")
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    (root / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    reads = simulate_snp_reads(ref, pos, alts, n_alts, N_READS, READ_LEN, 6)
    return root, ["".join("ACGT"[b - 1] for b in r) for r in reads]


def fastq_text(seqs, irregular=None):
    """Records of R bytes each; record `irregular` has its sequence on two lines (and a name one digit shorter: R bytes too)."""
    recs = []
    for i, s in enumerate(seqs):
        if i == irregular:
            recs.append(f"@r{i:05d}\n{s[:30]}\n{s[30:]}\n+\n{'I' * len(s)}\n")
        else:
            recs.append(f"@r{i:06d}\n{s}\n+\n{'I' * len(s)}\n")
    assert all(len(r) == R for r in recs)
    return "".join(recs).encode()


def record_inside_chunk(k):
    """A record in the middle of chunk k, wholly inside it and at least two records from either boundary."""
    i = (k * C + C // 2) // R
    assert k * C + 2 * R <= i * R and (i + 1) * R + 2 * R <= (k + 1) * C
    return i


def genotype(root, out, path, devices=None, env=None):
    r = _gram("genotype", "--gram_dir", str(root), "--reads", str(path), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", "6",
              "--genotype_dir", str(out), "--seed", "1234", *(["--devices", devices] if devices else []), env=env)
    print(r.stdout)
    return r


def outcome(r, out):
    return (r.returncode, [(out / "coverage" / f).read_bytes() for f in COVERAGE_FILES], [l for l in r.stdout.splitlines() if l.startswith("Count ")])


@pytest.mark.parametrize("devices", [None, "0,0"])
@pytest.mark.parametrize("route", ["text", "bgzf"])
def test_irregular_record_behind_delivered_chunks_is_fatal(sample, tmp_path, route, devices):
    """The record lies in chunk k = 3: the run ends with the number of reads mapped before it, which is the number of records
    that end inside chunks 0 .. k - 1, (k C) // R. Plain text is told to reformat; a BGZF file to decompress first."""
    root, seqs = sample
    k = 3
    text = fastq_text(seqs, irregular=record_inside_chunk(k))
    if route == "text":
        path, env = tmp_path / "r.fq", TEXT_ENV
        path.write_bytes(text)
    else:
        path, env = tmp_path / "r.fq.gz", BGZF_ENV
        path.write_bytes(bgzf(text, block=BLOCK))
    r = genotype(root, tmp_path / "out", path, devices, env)
    assert r.returncode != 0
    n = (k * C) // R if route == "text" else (k * MEMBERS * BLOCK) // R
    assert f"irregular FASTQ record after the first {n} reads" in r.stdout
    assert "reformat, or use a four-line FASTQ" in r.stdout
    assert ("decompress and reformat" in r.stdout) == (route == "bgzf")


@pytest.fixture(scope="module")
def irregular_first_chunk(sample, tmp_path_factory):
    """The file whose irregular record lies in the first chunk, as text and as BGZF, and what the host readers make of each."""
    root, seqs = sample
    d = tmp_path_factory.mktemp("first_chunk")
    text = fastq_text(seqs, irregular=record_inside_chunk(0))
    (d / "r.fq").write_bytes(text)
    (d / "r.fq.gz").write_bytes(bgzf(text, block=BLOCK))
    host = {}
    for name in ("r.fq", "r.fq.gz"):
        r = genotype(root, d / ("host_" + name), d / name, env={"GMX_HOST_GZ": "1"})
        host[name] = outcome(r, d / ("host_" + name))
    return d, host


@pytest.mark.parametrize("devices", [None, "0,0"])
@pytest.mark.parametrize("name,env", [("r.fq", TEXT_ENV), ("r.fq.gz", BGZF_ENV)])
def test_irregular_record_in_the_first_chunk_is_declined(sample, irregular_first_chunk, tmp_path, name, env, devices):
    """Nothing was delivered: the BGZF and the text routes decline without a word and the host readers take the file as if it
    had never been tried — status, coverage and counters are those of a run that keeps to the host (GMX_HOST_GZ=1). One engine
    tries a BGZF file the BGZF route declined as plain gzip next (a BGZF file is a gzip file), and that route hands every
    status to the host reader with a warning, also on its first chunk: "after 0 reads"."""
    root, _ = sample
    d, host = irregular_first_chunk
    r = genotype(root, tmp_path / "out", d / name, devices, env)
    if name == "r.fq.gz" and devices is None:
        assert "the device-side gzip decoder gave up after 0 reads; the host reader takes over" in r.stdout
        assert r.stdout.count("gave up after") == 1
    else:
        assert "gave up after" not in r.stdout
    assert "irregular FASTQ record after the first" not in r.stdout
    assert outcome(r, tmp_path / "out") == host[name]


def no_member_behind(seqs):
    """A BGZF FASTQ without its EOF marker, 64 bytes that are no member behind it."""
    return bgzf(fastq_text(seqs), block=BLOCK, eof=False) + b"\xaa" * 64


def test_bytes_that_are_no_member_behind_delivered_chunks(sample, tmp_path):
    """One engine walks the member table a chunk at a time: the walk of the LAST chunk meets the 64 bytes, so that chunk is
    never delivered; the chunks before it were. N is the number of records that end within them. The host reader takes the
    file over; its inflater, like gzip, stops at bytes behind the last member that are none, and the run ends well."""
    root, seqs = sample
    members = 30
    path = tmp_path / "r.fq.gz"
    path.write_bytes(no_member_behind(seqs))
    n_members = -(-N_READS * R // BLOCK)
    n_chunks = -(-n_members // members)
    assert n_chunks >= 4 and n_members % members  # (the last chunk is a short one: its walk runs into the 64 bytes)
    n = ((n_chunks - 1) * members * BLOCK) // R
    r = genotype(root, tmp_path / "out", path, env={"GMX_INGEST_MEMBERS": str(members)})
    assert f"BGZF decoder gave up after {n} reads; the host reader takes over" in r.stdout
    assert r.returncode == EXIT_NO_MEMBER_BEHIND


def test_bytes_that_are_no_member_behind_two_engines_decline(sample, tmp_path):
    """Two engines walk the whole table first: the file is declined before anything is delivered, without a warning, and the
    host reader reads it as above."""
    root, seqs = sample
    path = tmp_path / "r.fq.gz"
    path.write_bytes(no_member_behind(seqs))
    r = genotype(root, tmp_path / "out", path, "0,0", env={"GMX_INGEST_MEMBERS": "20"})
    assert "gave up after" not in r.stdout
    assert r.returncode == EXIT_NO_MEMBER_BEHIND


def test_bytes_that_are_no_member_at_offset_0_decline(sample, tmp_path):
    """The same 64 bytes at the head of a file named .gz: no route takes it (not BGZF, not gzip, no '@'), nothing is delivered,
    and the host readers are the ones to speak (`gram _parse_check`: their lines come first)."""
    _, seqs = sample
    path = tmp_path / "r.fq.gz"
    path.write_bytes(b"\xaa" * 64 + bgzf(fastq_text(seqs[:200]), block=BLOCK))
    r = _gram("_parse_check", str(path), "4", env={"GMX_PARSE_CHECK_DEVICE": "1"})
    print(r.stdout)
    assert r.returncode == 0
    assert "device declined after 0 reads" in r.stdout
    assert any(l.startswith("slow ") for l in r.stdout.splitlines())


EXIT_NO_MEMBER_BEHIND = 0  # (recorded: the host reader's inflater, like gzip, stops at bytes that are no member behind the last one)

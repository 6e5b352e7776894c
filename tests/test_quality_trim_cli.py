"""`gram genotype --trim_quality Q [--min_read_length M]`: the reads' 3' ends trimmed by quality before they are
mapped — on the device for FASTQ (plain, gzip, BGZF), in the host reader for BAM and on every host route. Against plain `gram
genotype` on the same reads cut in Python by the restated rule (tests/test_quality_trim_rule.py), route by route."""
import gzip
import json

import numpy as np
import pytest

from bam_common import bam_bytes, record, reverse_complement
from test_ingest import _gram, bgzf
from test_quality_trim_rule import trim_ref

pytestmark = pytest.mark.gpu

K = 6
Q = 20
COVERAGE = ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")


def fq_bytes(reads) -> bytes:
    return b"".join(f"@r{i}\n{s}\n+\n".encode() + q + b"\n" for i, (s, q) in enumerate(reads))


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """A flat PRG and 3 000 reads of 60 bases drawn from it. A third get 1-3 substitutions in their last 10 bases, quality '#' from
    the first of them on (every other one of those an N there too); every 50th read an error in its middle with good quality, which
    trimming must not rescue; every 97th a poor quality from base 1..5 on (it trims below k: skipped); every 41st an N in its middle."""
    from gramtools_amd.synth import random_ref, snp_prg, simulate_snp_reads
    d = tmp_path_factory.mktemp("trim_cli")
    rng = np.random.default_rng(2)
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    (d / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    drawn = simulate_snp_reads(ref, pos, alts, n_alts, 3000, 60, 6)
    other = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}
    reads = []
    for i, r in enumerate(drawn):
        s = list("".join("ACGT"[b - 1] for b in r))
        q = bytearray(b"I" * len(s))
        if i % 3 == 0:
            hit = sorted(rng.choice(np.arange(50, 60), int(rng.integers(1, 4)), replace=False))
            for k in hit:
                s[k] = other[s[k]][int(rng.integers(0, 3))]
            if i % 6 == 0:
                s[hit[-1]] = "N"
            q[hit[0]:] = b"#" * (len(s) - hit[0])
        elif i % 50 == 1:
            s[30] = other[s[30]][0]
        elif i % 97 == 2:
            k = int(rng.integers(1, K))
            q[k:] = b"#" * (len(s) - k)
        elif i % 41 == 4:
            s[20] = "N"
        reads.append(("".join(s), bytes(q)))
    cut = [(s[:trim_ref(q, Q)], q[:trim_ref(q, Q)]) for s, q in reads]
    ts = [len(s) for s, _ in cut]
    assert min(ts) >= 1  # (an empty sequence line is a malformed FASTQ record)
    assert any(t < K for t in ts) and len(set(ts)) > 5
    text = fq_bytes(reads)
    (d / "reads.fq").write_bytes(text)
    (d / "cut.fq").write_bytes(fq_bytes(cut))
    (d / "reads.bgzf.fq.gz").write_bytes(bgzf(text, block=9000))
    (d / "reads.fq.gz").write_bytes(gzip.compress(text, 6))
    records = []
    for i, (s, q) in enumerate(reads):  # every third record on the reverse strand: the file stores its reverse complement, qualities reversed
        phred = bytes(b - 33 for b in q)
        records.append(record(seq=reverse_complement(s), flag=0x10, name=f"r{i}", qual=phred[::-1]) if i % 3 == 1 else record(seq=s, name=f"r{i}", qual=phred))
    (d / "reads.bam").write_bytes(bgzf(bam_bytes(records), block=20000))
    stats = {"min_quality": Q, "min_length": K, "reads": len(reads), "reads_trimmed": sum(len(c[0]) < len(r[0]) for c, r in zip(cut, reads)),
             "bases_in": sum(len(r[0]) for r in reads), "bases_removed": sum(len(r[0]) - len(c[0]) for c, r in zip(cut, reads)),
             "reads_too_short": sum(t < K for t in ts)}
    return d, stats


_runs = {}


def run(sample, name, files, flags=(), env=None):
    """One `gram genotype` (cached by name): coverage files, the five counters, read_trim.json or None, the run's directory, its output."""
    d, _ = sample
    if name not in _runs:
        out = d / name
        r = _gram("genotype", "--gram_dir", str(d), "--reads", *[str(d / f) for f in files], "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", str(K),
                  "--genotype_dir", str(out), "--seed", "1234", *flags, env=env or {})
        assert r.returncode == 0, (name, r.stdout)
        counters = [l for l in r.stdout.splitlines() if l.startswith("Count ")]
        assert len(counters) == 5
        trim = json.loads((out / "read_trim.json").read_text()) if (out / "read_trim.json").exists() else None
        _runs[name] = ([(out / "coverage" / f).read_bytes() for f in COVERAGE], counters, trim, out, r.stdout)
    return _runs[name]


TRIM = ("--trim_quality", str(Q), "--min_read_length", str(K))


def mapped(counters):
    return int(counters[4].split(":")[1])


def test_trimmed_on_the_device_equals_the_file_cut_in_python(sample):
    """(a) coverage files and counters byte for byte; the per-read outcomes too."""
    cut = run(sample, "cut", ["cut.fq"], ("--read_outcomes",))
    on = run(sample, "on", ["reads.fq"], TRIM + ("--read_outcomes",))
    assert on[0] == cut[0] and on[1] == cut[1]
    assert (on[3] / "read_outcomes.bin").read_bytes() == (cut[3] / "read_outcomes.bin").read_bytes()
    assert on[2] == sample[1]
    assert cut[2] is None
    # --min_read_length defaults to the index's k
    dflt = run(sample, "default-min-length", ["reads.fq"], ("--trim_quality", str(Q)))
    assert dflt[:3] == on[:3]


def test_more_reads_map(sample):
    """(b) the point of it: reads with a miscalled tail map once the tail is gone; an error in good bases stays one."""
    off = run(sample, "off", ["reads.fq"])
    on = run(sample, "on", ["reads.fq"], TRIM + ("--read_outcomes",))
    assert mapped(on[1]) > mapped(off[1]) + 500  # (about 1 000 reads have a damaged tail)
    assert off[2] is None and not (off[3] / "read_trim.json").exists()
    assert on[0] != off[0]


@pytest.mark.parametrize("name,files,flags,env,says", [
    ("bgzf", ["reads.bgzf.fq.gz"], (), {"GMX_INGEST_MEMBERS": "7"}, None),
    ("gzip", ["reads.fq.gz"], (), {"GMX_GZ_CHUNK": "20000"}, None),
    ("text-64-threads", ["reads.fq"], ("--max_threads", "64"), {"GMX_TEXT_CHUNK": "50000"}, None),
    ("host-fastq", ["reads.fq"], (), {"GMX_HOST_FASTQ": "1"}, None),
    ("host-gz", ["reads.fq.gz"], (), {"GMX_HOST_GZ": "1"}, None),
    ("host-bgzf", ["reads.bgzf.fq.gz"], (), {"GMX_HOST_GZ": "1"}, None),
    ("takeover", ["reads.bgzf.fq.gz"], (), {"GMX_INGEST_MEMBERS": "20", "GMX_INGEST_TEST_FAIL_CHUNK": "2"}, "the host reader takes over"),
    ("takeover-text", ["reads.fq"], (), {"GMX_TEXT_CHUNK": "100000", "GMX_INGEST_TEST_FAIL_CHUNK": "1"}, "the host reader takes over"),
    ("two-engines", ["reads.bgzf.fq.gz"], ("--devices", "0,0"), {"GMX_INGEST_MEMBERS": "5"}, None),
    ("two-engines-text", ["reads.fq"], ("--devices", "0,0"), {"GMX_TEXT_CHUNK": "70000"}, None),
    ("bam", ["reads.bam"], (), {}, None),
    ("bam-two-engines", ["reads.bam"], ("--devices", "0,0"), {}, None),
])
def test_every_route_gives_the_same(sample, name, files, flags, env, says):
    """(c), (d) the device routes, the host routes, a take-over in the middle of the file (its reads counted once), chunks dealt over
    two engines, BAM with reverse-strand records through the host reader: coverage, counters and read_trim.json of the plain device run."""
    on = run(sample, "on", ["reads.fq"], TRIM + ("--read_outcomes",))
    got = run(sample, name, files, TRIM + tuple(flags), env)
    assert got[0] == on[0] and got[1] == on[1], name
    assert got[2] == on[2] == sample[1], name
    if says:
        assert says in got[4], got[4]


def test_two_files_and_a_samples_list(sample):
    """The counters add up over files; every sample of a list gets its own read_trim.json."""
    d, stats = sample
    both = run(sample, "two-files", ["reads.fq", "reads.bgzf.fq.gz"], TRIM)
    assert both[2] == {k: v if k.startswith("min_") else 2 * v for k, v in stats.items()}
    (d / "samples.tsv").write_text(f"a\t{d / 'list_a'}\t{d / 'reads.fq'}\nb\t{d / 'list_b'}\t{d / 'cut.fq'}\n")
    r = _gram("genotype", "--gram_dir", str(d), "--samples_list", str(d / "samples.tsv"), "--ploidy", "diploid", "--kmer_size", str(K), "--seed", "1234", *TRIM)
    assert r.returncode == 0, r.stdout
    on = run(sample, "on", ["reads.fq"], TRIM + ("--read_outcomes",))
    assert json.loads((d / "list_a" / "read_trim.json").read_text()) == stats
    second = json.loads((d / "list_b" / "read_trim.json").read_text())  # the cut file: nothing left to trim, the short reads still short
    assert second["reads_trimmed"] == 0 and second["bases_removed"] == 0 and second["reads_too_short"] == stats["reads_too_short"]
    assert second["bases_in"] == stats["bases_in"] - stats["bases_removed"]
    for name in ("list_a", "list_b"):
        assert [(d / name / "coverage" / f).read_bytes() for f in COVERAGE] == on[0]


@pytest.mark.parametrize("flags", [("--trim_quality", "0"), ("--trim_quality", "94"), ("--trim_quality", "x"), ("--trim_quality", "20.5"), ("--trim_quality", ""),
                                   ("--trim_quality", "20", "--min_read_length", "0"), ("--trim_quality", "20", "--min_read_length", "-3"),
                                   ("--trim_quality", "20", "--min_read_length", "ten"), ("--min_read_length", "10")])
def test_bad_values_end_the_run(sample, flags):
    """(e) exit 1 with a message, before an engine exists."""
    d, _ = sample
    r = _gram("genotype", "--gram_dir", str(d), "--reads", str(d / "reads.fq"), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", str(K),
              "--genotype_dir", str(d / "bad"), "--seed", "1", *flags)
    assert r.returncode == 1, r.stdout
    assert "--trim_quality" in r.stdout or "--min_read_length" in r.stdout
    assert "Loading PRG data" not in r.stdout


def test_without_the_flag_nothing_changes(sample):
    """(f) no read_trim.json; two runs give the same bytes; and with the flag on reads that have nothing to trim, every coverage and
    genotype file is the one the run without the flag writes."""
    d, _ = sample
    off = run(sample, "off", ["reads.fq"])
    again = run(sample, "off-again", ["reads.fq"])
    names = ["coverage/" + f for f in COVERAGE] + ["genotype/genotyped.json", "genotype/genotyped.vcf.gz", "genotype/personalised_reference.fasta", "read_stats.json"]
    for n in names:
        assert (off[3] / n).read_bytes() == (again[3] / n).read_bytes(), n
    assert not (off[3] / "read_trim.json").exists() and not (again[3] / "read_trim.json").exists()
    good = run(sample, "cut-on", ["cut.fq"], ("--trim_quality", str(Q), "--min_read_length", "1"))
    plain = run(sample, "cut", ["cut.fq"], ("--read_outcomes",))
    for n in names:
        assert (good[3] / n).read_bytes() == (plain[3] / n).read_bytes(), n
    assert good[1] == plain[1] and good[2]["reads_trimmed"] == 0 and good[2]["reads_too_short"] == 0
    # read_stats.json is computed on the reads as they lie in the file, whatever the flag
    on = run(sample, "on", ["reads.fq"], TRIM + ("--read_outcomes",))
    stats_on, stats_off = (json.loads((r[3] / "read_stats.json").read_text()) for r in (on, off))
    assert stats_on["Max_read_length"] == stats_off["Max_read_length"] == 60 and stats_on["Quality"] == stats_off["Quality"]

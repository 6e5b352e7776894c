"""The grouped log per strand (GMX_LOG_REVERSE, gmx_coverage_fetch_grouped_log_strand, include/gmx.h) and `gram genotype
--strand_bias`. A task's strand rides in bit 30 of its log records' second word; the engine keeps two counts per distinct
(site, ids), the exchange carries both, and the infer stage turns them into COV_FWD, COV_REV and SB.

The oracle for one strand is the oracle itself, as in test_strand_coverage.py: Oracle.quasimap_read maps ONE orientation."""
import ctypes as C
import gzip
import json

import numpy as np
import pytest

from common import flatten_reads
from oracle import Oracle
from gramtools_amd import GmxError, Index, Quasimapper, QuasimapperGroup, _lib, master_seeds
from gramtools_amd.quasimap import LOG_COUNTED, LOG_REVERSE, iter_grouped_log
from gramtools_amd.synth import random_ref, simulate_snp_reads, snp_prg
from strand_bias_common import counted, expected_fields, strip_json, strip_vcf
from test_many_instances import tandem_prg, tandem_reads
from test_strand_coverage import feed, flat_case, log_case, log_sites_of, revcomp, run

pytestmark = pytest.mark.gpu

GMX_EINVAL = -1


def decoded(log):
    """{(site, ids): count} of a log of counted records, one per key."""
    out = {}
    for s, ids, count in iter_grouped_log(log):
        assert (s, ids) not in out and count > 0
        out[(s, ids)] = count
    return out


def oracle_logs(prg, k, reads, seeds, log_sites):
    """Per orientation: {(site, ids): count} at the sites on the log, from Oracle.quasimap_read over the reads as given (0) and
    over their reverse complements (1)."""
    out = []
    for strand in (0, 1):
        o = Oracle(prg, k)
        for r, s in zip(reads, seeds):
            o.quasimap_read(revcomp(r) if strand else np.asarray(r, dtype=np.uint8), int(s))
        grouped = o.grouped()
        out.append({(s, ids): c for s in log_sites for ids, c in grouped[s].items()})
        o.close()
    return out


def check_log_split(prg, k, reads, seeds, **kw):
    ix = Index(prg, k)
    sites = log_sites_of(ix)
    assert sites
    want = oracle_logs(prg, k, reads, seeds, sites)
    qm = run(ix, reads, seeds, **kw)
    got = [decoded(qm.grouped_log(strand=s)) for s in (0, 1)]
    assert got[0] == want[0], "forward log"
    assert got[1] == want[1], "reverse log"
    assert got[0] and got[1]  # (records written to the wrong strand cannot hide)
    total = qm.grouped_log()
    plain = run(ix, reads, seeds, strands=False, **kw).grouped_log()
    assert total.size and total.tolist() == plain.tolist()  # word for word
    assert not any(int(w) & LOG_REVERSE for _, w in second_words(total))
    tot = decoded(total)
    assert set(tot) == set(got[0]) | set(got[1])
    for key, c in tot.items():
        assert got[0].get(key, 0) + got[1].get(key, 0) == c, key
    return ix, qm


def second_words(log):
    i = 0
    while i < len(log):
        w = int(log[i + 1])
        yield i, w
        i += (4 if w & LOG_COUNTED else 2) + (w & ~(LOG_COUNTED | LOG_REVERSE))


# ---- T1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense_max", [None, "2"], ids=["one-log-site", "every-multi-allelic-site"])
def test_the_log_split_against_the_per_orientation_oracle(monkeypatch, dense_max):
    if dense_max:
        monkeypatch.setenv("GMX_DENSE_MAX_ALLELES", dense_max)
    prg, k, reads = flat_case()
    seeds = (np.arange(len(reads), dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)
    ix, qm = check_log_split(prg, k, reads, seeds)
    assert len(log_sites_of(ix)) == (1 if dense_max is None else 8)
    # the accessors above the C call
    fwd = qm.coverage(strand=0)
    assert fwd.raw_grouped_log.size == 0
    whole = fwd.with_grouped_log(qm.grouped_log(strand=0))
    site = log_sites_of(ix)[-1]
    assert whole.grouped_allele_counts[site] == {ids: c for (s, ids), c in decoded(qm.grouped_log(strand=0)).items() if s == site}
    with pytest.raises(ValueError):
        qm.grouped_log(strand=2)


# ---- T2 --------------------------------------------------------------------------------------------------------------
def test_a_replayed_task_logs_into_its_own_strand(monkeypatch):
    """A log of 64 words and batches of 150 reads: tasks that find the log full are redone whole after a drain, from queue
    entries that carry the task id — the redone records carry the same bit."""
    prg, k, reads = log_case()
    ix = Index(prg, k)
    assert ix.uses_grouped_log
    seeds = master_seeds(5, [len(reads)])
    roomy = run(ix, reads, seeds)
    assert roomy.queue_counts()["log_replays"] == 0
    tiny = run(ix, reads, seeds, chunk=300, log_cap_words=64, max_batch_reads=150)
    assert tiny.queue_counts()["log_replays"] > 0
    for s in (0, 1):
        want = roomy.grouped_log(strand=s)
        assert want.size and tiny.grouped_log(strand=s).tolist() == want.tolist(), s
    assert tiny.grouped_log().tolist() == roomy.grouped_log().tolist()


# ---- T3 --------------------------------------------------------------------------------------------------------------
# flat_case()'s first 20 reads, seeds 7 * i + 1, every multi-allelic site on the log (GMX_DENSE_MAX_ALLELES=2), recording off: the
# totals log as the engine returned it before records had a strand (counted records in key order; the counts are the oracle's)
def t3_case():
    prg, k, reads = flat_case()
    reads = reads[:20]
    seeds = (np.arange(20, dtype=np.uint32) * 7 + 1).astype(np.uint32)
    return prg, k, reads, seeds


K = LOG_COUNTED
T3_LITERAL = [9, 1 | K, 1, 0, 0, 9, 1 | K, 1, 0, 3, 13, 1 | K, 1, 0, 1, 13, 1 | K, 1, 0, 2, 19, 1 | K, 1, 0, 1, 20, 1 | K, 1, 0, 5]


def test_with_recording_off_no_record_has_a_strand(monkeypatch):
    """No call returns the device log's raw words, so "bit 30 is never set" is checked through the host's drain: it refuses a
    record with the bit from an engine that does not record strands (GMX_EREF, an invariant check this change adds), and sums
    by key otherwise. A totals fetch that succeeds and equals the literal has therefore seen no such record."""
    monkeypatch.setenv("GMX_DENSE_MAX_ALLELES", "2")
    prg, k, reads, seeds = t3_case()
    ix = Index(prg, k)
    qm = run(ix, reads, seeds, strands=False)
    lib = qm.lib
    got = qm.grouped_log()
    assert got.tolist() == T3_LITERAL
    assert qm.export_grouped_log().tolist() == T3_LITERAL
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    buf = np.zeros(64, dtype=np.uint32)
    assert lib.gmx_coverage_fetch_grouped_log_strand(qm.h, 0, u32(buf), 64) == GMX_EINVAL and b"record" in lib.gmx_last_error()
    assert lib.gmx_coverage_fetch_grouped_log_strand(qm.h, 1, None, 0) == GMX_EINVAL
    assert lib.gmx_coverage_fetch_grouped_log_strand(None, 0, None, 0) == GMX_EINVAL
    with pytest.raises(GmxError):
        qm.grouped_log(strand=0)
    for rec in ([20, 1 | LOG_REVERSE, 3], [20, 1 | LOG_COUNTED | LOG_REVERSE, 2, 0, 3], [20, 1, 4, 20, 1 | LOG_REVERSE, 3]):
        r = np.asarray(rec, dtype=np.uint32)
        assert lib.gmx_coverage_import_grouped_log(qm.h, u32(r), r.size, 0) == GMX_EINVAL, rec
        assert lib.gmx_coverage_import_grouped_log(qm.h, u32(r), r.size, 1) == GMX_EINVAL, rec
    assert qm.grouped_log().tolist() == T3_LITERAL  # a refused import changes nothing, with `replace` too
    on = run(ix, reads, seeds)
    assert lib.gmx_coverage_fetch_grouped_log_strand(on.h, 2, None, 0) == GMX_EINVAL
    assert lib.gmx_coverage_fetch_grouped_log_strand(on.h, -1, None, 0) == GMX_EINVAL
    assert on.grouped_log().tolist() == T3_LITERAL


# ---- T4 --------------------------------------------------------------------------------------------------------------
def test_export_and_import_carry_both_strands():
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    a = run(ix, reads, seeds)
    want = [a.grouped_log(strand=s) for s in (0, 1)]
    exported = a.export_grouped_log()
    assert [bool(w & LOG_REVERSE) for _, w in second_words(exported)].count(True) == len(decoded(want[1]))
    assert all(w & LOG_COUNTED for _, w in second_words(exported))
    b = Quasimapper(ix)
    b.record_strands(True)
    feed(b, reads[:50], seeds[:50])  # something to replace
    b.import_grouped_log(exported, replace=True)
    for s in (0, 1):
        assert b.grouped_log(strand=s).tolist() == want[s].tolist()
    assert b.grouped_log().tolist() == a.grouped_log().tolist()
    b.import_grouped_log(exported)
    for s in (0, 1):
        assert decoded(b.grouped_log(strand=s)) == {key: 2 * c for key, c in decoded(want[s]).items()}
    # the plain record form, with and without the bit, on top
    b.import_grouped_log(np.asarray([20, 2 | LOG_REVERSE, 1, 5, 20, 2, 1, 5, 20, 2 | LOG_REVERSE, 1, 5], dtype=np.uint32), replace=True)
    assert b.grouped_log(strand=0).tolist() == counted(20, (1, 5), 1) and b.grouped_log(strand=1).tolist() == counted(20, (1, 5), 2)
    assert b.grouped_log().tolist() == counted(20, (1, 5), 3)
    b.reset()
    assert b.grouped_log(strand=0).size == 0 and b.grouped_log(strand=1).size == 0 and b.grouped_log().size == 0


# ---- T5 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forward_only", [False, True], ids=["both-orientations", "forward-only"])
def test_a_group_exchanges_both_strands_logs(forward_only):
    """Two engines on device 0: the exchange's peer-copy fallback (RCCL needs distinct devices)."""
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    kw = dict(forward_only=True) if forward_only else {}
    single = run(ix, reads, seeds, **kw)
    want = [single.grouped_log(strand=s) for s in (0, 1)]
    assert want[0].size and (want[1].size == 0) == forward_only
    flat, offs = flatten_reads(reads)
    grp = QuasimapperGroup(ix, [0, 0], **kw)
    assert not grp.uses_rccl
    grp.record_strands(True)
    grp.map_reads(flat, offs, seeds)
    grp.allreduce()
    for member in (0, 1):
        for s in (0, 1):
            assert grp.grouped_log(member, strand=s).tolist() == want[s].tolist(), (member, s)
        assert grp.grouped_log(member).tolist() == single.grouped_log().tolist()
        assert grp.export_grouped_log(member).tolist() == single.export_grouped_log().tolist()
    grp.close()


# ---- T6 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_copies", [10, 300], ids=["cooperative", "large-capacity-tier"])
def test_the_general_instances_log_with_the_tasks_strand(monkeypatch, n_copies):
    """Tandem copies of a unit with a two-allele site: a read has one mapping instance per copy, recorded by the cooperative
    and serial general instances (10 copies) and the large-capacity pass (300). GMX_DENSE_MAX_ALLELES=1: sites of up to that
    many alleles keep dense counters, so 1 — not 2 — is what puts these two-allele sites on the log."""
    monkeypatch.setenv("GMX_DENSE_MAX_ALLELES", "1")
    prg, unit, site_at, alt = tandem_prg(n_copies, 60, 5)
    reads = tandem_reads(unit, site_at, alt, 100, 6)
    seeds = master_seeds(11, [len(reads)])
    ix, qm = check_log_split(prg, 8, reads, seeds)
    assert len(log_sites_of(ix)) == n_copies
    counts = qm.queue_counts()
    if n_copies == 10:
        assert counts["cover_general"] > 0 and counts["big_mapped"] >= 4, counts
    else:
        assert counts["big_mapped"] + counts["cover_overflow"] > 0, counts


# ---- T7, T8: gram genotype --strand_bias -----------------------------------------------------------------------------
def make_sample(d, prg, reads):
    from test_ingest import bgzf
    (d / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    txt = ["".join("ACGT"[b - 1] for b in r) for r in reads]
    fq = "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(txt)).encode()
    (d / "s.fq").write_bytes(fq)
    (d / "s.bgzf.fq.gz").write_bytes(bgzf(fq, block=9000))


def strand_groups(ix, reads, seed):
    """Per strand, per site {ids: raw count}: the engine's own strand fetches for these reads and master_seeds(seed)."""
    qm = run(ix, list(reads), master_seeds(seed, [len(reads)]))
    out = []
    for s in (0, 1):
        cov = qm.coverage(strand=s)
        sites = [dict() for _ in range(ix.n_sites)]
        for i in range(ix.n_sites):
            off, n = int(ix.grouped_off[i]), int(ix.n_alleles[i])
            if i in log_sites_of(ix):
                continue
            vals = cov.raw_grouped[off:off + (1 << n) - 1]
            for m in np.nonzero(vals)[0]:
                sites[i][tuple(a for a in range(n) if ((int(m) + 1) >> a) & 1)] = int(vals[m])
        for i, ids, c in iter_grouped_log(qm.grouped_log(strand=s)):
            sites[i][ids] = sites[i].get(ids, 0) + c
        out.append(sites)
    return out


def site_alleles(prg):
    """Per site of a flat PRG: its alleles' sequences, in order (site marker m, then every allele closed by m + 1)."""
    ints = [int(x) for x in prg]
    sites = []
    for m in sorted({x for x in ints if x > 4 and x % 2 == 1}):
        cuts = [ints.index(m)] + [i for i, x in enumerate(ints) if x == m + 1]
        sites.append(["".join("ACGT"[x - 1] for x in ints[lo + 1:hi]) for lo, hi in zip(cuts, cuts[1:])])
    return sites


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from ingest_formats_common import gram
    cases = {}
    # the 3 kb / 40-site sample of test_strand_coverage.py's CLI tests
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    reads = simulate_snp_reads(ref, pos, alts, n_alts, 6100, 60, 6)
    cases["snp"] = (tmp_path_factory.mktemp("strand_bias_snp"), np.asarray(prg, dtype=np.uint32), list(reads))
    # a PRG with a 9-allele site: its grouped counts travel on the log
    prg9, k9, reads9 = flat_case()
    cases["nine"] = (tmp_path_factory.mktemp("strand_bias_nine"), prg9, reads9 * 6)
    for d, prg, reads in cases.values():
        make_sample(d, prg, reads)

    def run_gram(case, name, reads_file="s.fq", extra=()):
        d = cases[case][0]
        out = d / name
        if not out.exists():
            r = gram("genotype", "--gram_dir", str(d), "--reads", str(d / reads_file), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", "6",
                     "--genotype_dir", str(out), "--seed", "1234", *extra)
            assert r.returncode == 0, (name, r.stdout)
        return out

    groups = {}

    def groups_of(case):
        if case not in groups:
            _, prg, reads = cases[case]
            groups[case] = (strand_groups(Index(prg, 6), reads, 1234), site_alleles(prg))
        return groups[case]

    return dict(run=run_gram, groups=groups_of, dir=lambda case: cases[case][0])


def files_of(out):
    return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}


def check_calls(out, groups, alleles):
    j = json.loads((out / "genotype" / "genotyped.json").read_text())
    assert {"COV_FWD", "COV_REV", "SB"} <= set(j["Site_Fields"])
    n_called = 0
    for i, s in enumerate(j["Sites"]):
        if s["GT"][0][0] is None:
            assert s["SB"] == [None] and s["COV_FWD"] == [[]] and s["COV_REV"] == [[]]
            continue
        n_called += 1
        want = expected_fields(s, groups[0][i], groups[1][i], [alleles[i].index(a) for a in s["ALS"]])
        assert s["COV_FWD"] == [want["COV_FWD"]] and s["COV_REV"] == [want["COV_REV"]], (i, s, want)
        assert abs(s["SB"][0] - want["SB"]) <= 1e-6, (i, s, want)
    return j, n_called


@pytest.mark.parametrize("case,name,reads_file,extra", [("snp", "plain", "s.fq", []), ("snp", "bgzf", "s.bgzf.fq.gz", []),
                                                         ("snp", "two-engines", "s.fq", ["--devices", "0,0"]),
                                                         ("nine", "log-site", "s.fq", []), ("nine", "log-site-two-engines", "s.fq", ["--devices", "0,0"])])
def test_gram_strand_bias(cli, case, name, reads_file, extra):
    out = cli["run"](case, name, reads_file, ["--strand_bias", *extra])
    base = cli["run"](case, name + "-noflag", reads_file, extra)
    groups, alleles = cli["groups"](case)
    j, n_called = check_calls(out, groups, alleles)
    assert n_called >= (30 if case == "snp" else 10)
    if case == "nine":
        assert len(alleles[-1]) == 9 and sum(map(sum, (g[-1].values() for g in groups))) > 0  # the log site has counts on the log
    with_flag, without = files_of(out), files_of(base)
    assert sorted(with_flag) == sorted(without) and len(without) >= 6
    assert not any(".forward" in rel or ".reverse" in rel for rel in with_flag)
    for rel in without:
        if rel.endswith("genotyped.json"):
            assert strip_json(with_flag[rel].decode()) == without[rel].decode() and with_flag[rel] != without[rel]
        elif rel.endswith("genotyped.vcf.gz"):
            assert strip_vcf(gzip.decompress(with_flag[rel]).decode()) == gzip.decompress(without[rel]).decode()
        else:  # every other file of the run (read_stats.json, coverage/*, the personalised reference): as it is
            assert with_flag[rel] == without[rel], rel
    vcf = gzip.decompress(with_flag["genotype/genotyped.vcf.gz"]).decode().splitlines()
    recs = [l.split("\t") for l in vcf if not l.startswith("#")]
    assert len(recs) == len(j["Sites"]) and all(r[8].endswith(":COV_FWD:COV_REV:SB") for r in recs)
    for r, s in zip(recs, j["Sites"]):
        f = dict(zip(r[8].split(":"), r[9].split(":")))
        if s["GT"][0][0] is None:
            assert (f["COV_FWD"], f["COV_REV"], f["SB"]) == (".", ".", ".")
        else:
            assert f["COV_FWD"] == ",".join(map(str, s["COV_FWD"][0])) and f["COV_REV"] == ",".join(map(str, s["COV_REV"][0]))
            assert float(f["SB"]) == pytest.approx(s["SB"][0], rel=1e-5, abs=1e-30)


def test_gram_strand_bias_with_strand_coverage_does_both(cli):
    out = cli["run"]("snp", "both-flags", "s.fq", ["--strand_bias", "--strand_coverage"])
    alone = cli["run"]("snp", "plain", "s.fq", ["--strand_bias"])
    both, one = files_of(out), files_of(alone)
    extra = sorted(set(both) - set(one))
    assert extra == ["coverage/allele_base_coverage.forward.json", "coverage/allele_base_coverage.reverse.json",
                     "coverage/allele_sum_coverage.forward", "coverage/allele_sum_coverage.reverse"]
    for rel in ("genotype/genotyped.json", "genotype/genotyped.vcf.gz", "coverage/grouped_allele_counts_coverage.json"):
        assert both[rel] == one[rel], rel


def test_gram_strand_bias_across_a_samples_list(cli, tmp_path):
    """Two samples in one call: each sample's calls are those of a call of its own."""
    from ingest_formats_common import gram
    d = cli["dir"]("snp")
    own = {"a": cli["run"]("snp", "plain", "s.fq", ["--strand_bias"]), "b": cli["run"]("snp", "bgzf", "s.bgzf.fq.gz", ["--strand_bias"])}
    lst = tmp_path / "samples.tsv"
    lst.write_text(f"a\t{tmp_path / 'a'}\t{d / 's.fq'}\nb\t{tmp_path / 'b'}\t{d / 's.bgzf.fq.gz'}\n")
    r = gram("genotype", "--gram_dir", str(d), "--samples_list", str(lst), "--ploidy", "diploid", "--kmer_size", "6", "--seed", "1234", "--strand_bias")
    assert r.returncode == 0, r.stdout
    for s in ("a", "b"):
        got = json.loads((tmp_path / s / "genotype" / "genotyped.json").read_text())
        want = json.loads((own[s] / "genotype" / "genotyped.json").read_text())
        got["Samples"][0]["Name"] = want["Samples"][0]["Name"]  # (the list names the samples a and b)
        assert got == want and "SB" in got["Sites"][0]

"""Per-read positions (gmx_engine_record_positions, include/gmx.h): four uint32 per read — [pos, n] of the read as
given, [pos, n] of its reverse complement. n is the number of mapping instances (one per suffix-array index of every final
search state), pos the smallest PRG position among the instances the selection chose from. The expected record comes from the
oracle alone: its search, its class map, its draw and its suffix array. Compared read by read, and between the feeds, the
workspaces, the capacity tiers, the log replay, engine groups and the routes of `gram genotype --read_positions`."""
import ctypes as C
import functools
import json
import struct

import numpy as np
import pytest

from common import flatten_reads
from oracle import Oracle
from oracle.oracle import RNG_LEMIRE
from gramtools_amd import Index, Quasimapper, master_seeds, pack_reads
from gramtools_amd.synth import random_ref, simulate_snp_reads, snp_prg
from test_many_instances import tandem_prg, tandem_reads
from test_read_outcomes import FEEDS, flat_case, nested_case, repeat_case, revcomp, run_feed, tiled

pytestmark = pytest.mark.gpu


# ---- the oracle's record ---------------------------------------------------------------------------------------------
def oracle_task(o, sa, k, read, seed, mode=RNG_LEMIRE):
    """(pos, n, what) of ONE oriented read. `what` describes the task for the cases' own counts: the positions of all its
    instances, nonvar, the number of classes and the number drawn (0: no draw)."""
    read = np.asarray(read, dtype=np.uint8)
    if read.size < max(k, 1) or ((read < 1) | (read > 4)).any():
        return 0, 0, None
    states = o.search_read_backwards(read)
    if not states:
        return 0, 0, None
    n = sum(hi - lo + 1 for lo, hi, _, _ in states)
    everything = [int(sa[i]) for lo, hi, _, _ in states for i in range(lo, hi + 1)]
    nonvar, entries = o.unique_site_paths(states)
    r = 0
    if not entries:
        cand = everything
    else:
        r = int(Oracle.rng_generate(int(seed), 1, nonvar + len(entries), 1, mode)[0])
        if r <= nonvar:  # the non-variant instances: the path-less states the encapsulation leaves outside every site
            cand = [int(sa[i]) for lo, hi, tvd, tvg in o.encapsulated(states) if not tvd and not tvg for i in range(lo, hi + 1)]
            assert len(cand) == nonvar
        else:
            cand = [int(sa[i]) for lo, hi in entries[r - nonvar - 1][1] for i in range(lo, hi + 1)]
    return min(cand), min(n, 0xFFFFFFFF), dict(positions=everything, nonvar=nonvar, classes=len(entries), r=r)


def oracle_records(prg, k, reads, seeds, forward_only=False):
    o = Oracle(prg, k)
    sa = o.sa()
    out = np.zeros((len(reads), 4), dtype=np.uint32)
    what = []
    for i, r in enumerate(reads):
        r = np.asarray(r, dtype=np.uint8)
        pf, nf, wf = oracle_task(o, sa, k, r, seeds[i])
        pr, nr, wr = (0, 0, None) if forward_only else oracle_task(o, sa, k, Oracle.reverse_complement(r) if r.size else r, seeds[i])
        out[i] = (pf, nf, pr, nr)
        what += [wf, wr]
    o.close()
    return out, what


def default_seeds(n):
    return master_seeds(7, [n])


def record(ix, reads, seeds=None, feed="bytes", chunk=0, **kw):
    """The position records, the outcome bytes and the engine of `reads` through one feed, `chunk` reads per launch."""
    qm = Quasimapper(ix, **kw)
    qm.record_positions(True)
    qm.record_outcomes(True)
    run_feed(qm, reads, seeds if seeds is not None else default_seeds(len(reads)), feed, chunk)
    return qm.positions(), qm.outcomes(), qm


def assert_same(got, want, note=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint32, (got.shape, want.shape, got.dtype)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (note, [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:10]])


def check_outcome_codes(pos, out):
    """n > 0 exactly where the outcome code is 3, and pos is 0 where n is 0."""
    out = np.asarray(out, dtype=np.uint8)
    assert ((pos[:, 1] > 0) == ((out & 3) == 3)).all() and ((pos[:, 3] > 0) == (((out >> 2) & 3) == 3)).all()
    assert (pos[pos[:, 1] == 0, 0] == 0).all() and (pos[pos[:, 3] == 0, 2] == 0).all()


@functools.lru_cache(maxsize=None)
def case(name):
    """(prg, k, reads, seeds, the oracle's records, the oracle's description of every task), computed once."""
    prg, k, reads = {"flat": flat_case, "nested": nested_case, "repeat": repeat_case, "half_sited": half_sited_case}[name]()
    seeds = np.arange(1, len(reads) + 1, dtype=np.uint32) if name == "half_sited" else default_seeds(len(reads))
    want, what = oracle_records(prg, k, reads, seeds)
    return prg, k, reads, seeds, want, what


def check_case(name):
    prg, k, reads, seeds, want, what = case(name)
    got, out, qm = record(Index(prg, k), reads, seeds)
    assert qm.position_count() == len(reads)
    assert_same(got, want, name)
    check_outcome_codes(got, out)
    return got, out


def half_sited_case():
    """Ten tandem copies of a 60-base unit between unique flanks of 200; the EVEN copies carry a two-allele SNP site at base 30, the
    odd ones do not. A read of the all-reference haplotype over base 30 has five non-variant instances (the odd copies) and five
    classes (the even copies' sites): the draw falls on the lump of non-variant instances or on a class."""
    rng = np.random.default_rng(11)
    unit = rng.integers(1, 5, size=60, dtype=np.uint8)
    left, right = rng.integers(1, 5, size=200, dtype=np.uint8), rng.integers(1, 5, size=200, dtype=np.uint8)
    alt = int(unit[30]) % 4 + 1
    prg, hap, m = [int(x) for x in left], [int(x) for x in left], 5
    for c in range(10):
        hap += [int(x) for x in unit]
        if c % 2 == 0:
            prg += [int(x) for x in unit[:30]] + [m, int(unit[30]), m + 1, alt, m + 1] + [int(x) for x in unit[31:]]
            m += 2
        else:
            prg += [int(x) for x in unit]
    prg += [int(x) for x in right]
    hap = np.asarray(hap + [int(x) for x in right], dtype=np.uint8)
    reads = []
    for j in range(200):
        st = int(rng.integers(0, hap.size - 30 + 1))
        r = hap[st:st + 30].copy()
        reads.append(revcomp(r) if j % 2 else r)
    return np.asarray(prg, dtype=np.uint32), 6, reads


# ---- read by read against the oracle ---------------------------------------------------------------------------------
def test_flat_prg_read_by_read_against_the_oracle():
    prg, k, reads, seeds, want, _ = case("flat")
    got, _ = check_case("flat")
    assert (want[:, 1] > 0).sum() > 100 and (want[:, 1] == 0).sum() > 10
    # the record of revcomp(read) is the read's record with the two halves swapped
    clean = [i for i, r in enumerate(reads) if len(r) and ((np.asarray(r) >= 1) & (np.asarray(r) <= 4)).all()]
    rc, _, _ = record(Index(prg, k), [revcomp(reads[i]) for i in clean], seeds[clean])
    assert_same(rc, got[clean][:, [2, 3, 0, 1]], "reverse complements")


def test_nested_prg_counts_instances_not_positions():
    _, _, _, _, want, what = case("nested")
    several = [w for w in what if w and len(w["positions"]) > 1]
    shared = [w for w in several if len(set(w["positions"])) < len(w["positions"])]  # two states at one text position
    assert len(several) >= 20 and len(shared) >= 10, (len(several), len(shared))
    check_case("nested")


def test_repeats_draw_among_classes_or_report_every_copy():
    prg, k, reads, seeds, want, what = case("repeat")
    drawn = [t for t, w in enumerate(what) if w and w["classes"] and w["nonvar"] + w["classes"] > 1]
    no_class = [t for t, w in enumerate(what) if w and not w["classes"] and w["nonvar"] > 1]
    assert len(drawn) >= 40 and len(no_class) >= 30, (len(drawn), len(no_class))
    got, out = check_case("repeat")
    for t in no_class:  # several non-variant copies, no class: no draw — the smallest position, their number, no multi bit
        w = what[t]
        assert got[t >> 1, 2 * (t & 1)] == min(w["positions"]) and got[t >> 1, 2 * (t & 1) + 1] == len(w["positions"]) == w["nonvar"]
        assert not (int(out[t >> 1]) >> (4 + (t & 1))) & 1
    # a read over the site, mapped alone: the site that got its coverage lies within one read length of pos
    _, unit, site_at, _ = tandem_prg(10, 60, 8, flank=200)
    inside = np.tile(unit, 2)[site_at - 10:site_at + 20]
    for seed in (1, 2, 3, 4, 5):
        pos, _, qm = record(Index(prg, k), [inside], np.asarray([seed], dtype=np.uint32), forward_only=True)
        assert pos[0, 1] == 10 and pos[0, 3] == 0
        covered = [s for s, alleles in enumerate(qm.coverage().allele_sum_coverage) if any(alleles)]
        assert len(covered) == 1
        marker_at = int(np.flatnonzero(np.asarray(prg) == 5 + 2 * covered[0])[0])
        assert abs(marker_at - int(pos[0, 0])) <= len(inside), (seed, marker_at, pos[0].tolist())


def test_half_sited_repeat_pins_the_lump_of_non_variant_instances():
    _, _, _, _, want, what = case("half_sited")
    mixed = [w for w in what if w and w["classes"] and w["nonvar"]]
    lump = [w for w in mixed if w["r"] <= w["nonvar"]]
    a_class = [w for w in mixed if w["r"] > w["nonvar"]]
    assert len(lump) >= 15 and len(a_class) >= 15, (len(mixed), len(lump), len(a_class))
    check_case("half_sited")


# ---- feeds, workspaces, resets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("twin", ["0", "1"])
def test_every_route_gives_the_same_records(monkeypatch, twin):
    import torch
    monkeypatch.setenv("GMX_TWIN", twin)
    prg, k, reads, _, _, _ = case("flat")
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    want, _, _ = record(ix, reads, seeds)
    assert (want[:, 1] > 0).sum() > 100
    for feed in FEEDS:
        for chunk in (0, 97):
            got, _, qm = record(ix, reads, seeds, feed=feed, chunk=chunk)
            assert bool(qm.lib.gmx_engine_second_stream(qm.h)) == (twin == "1")
            assert_same(got, want, (feed, chunk))
            if chunk:  # a queued reset: the count starts again, nothing of the reads before shows
                qm.reset(stream=torch.cuda.current_stream().cuda_stream)
                assert qm.position_count() == 0
                run_feed(qm, reads[100:], seeds[100:], feed, chunk)
                assert qm.position_count() == len(reads) - 100
                assert_same(qm.positions(), want[100:], (feed, "after reset"))
                assert_same(qm.positions(5, 40), want[105:145], (feed, "slice"))
                qm.reset()
                assert qm.position_count() == 0
                run_feed(qm, reads[:50], seeds[:50], feed, chunk)
                assert_same(qm.positions(), want[:50], (feed, "after the second reset"))


def test_a_full_buffer_grows_and_carries_the_records_over(monkeypatch):
    """The buffer starts at 1 MiB, 65 536 records. Four launches of 27 copies of the first 611 reads of the flat case, 16 497 reads
    each: the fourth needs 65 988 records and makes the buffer grow with 49 491 recorded. With GMX_TWIN=1 the launch before may
    still be in flight on the other workspace. Every record is the oracle's for its read and seed (it depends on nothing else), a
    slice across the carried / new boundary too; a reset clears the grown buffer."""
    monkeypatch.setenv("GMX_TWIN", "1")
    prg, k, reads, seeds, want, _ = case("flat")
    reads, seeds, want = reads[:611], seeds[:611], want[:611]
    copies, launches = 27, 4
    per_launch = copies * len(reads)
    assert (launches - 1) * per_launch < (1 << 16) < launches * per_launch
    flat, offs, s = tiled(reads, seeds, copies)
    qm = Quasimapper(Index(prg, k))
    qm.record_positions(True)
    assert qm.lib.gmx_engine_second_stream(qm.h)
    for _ in range(launches):
        qm.map_reads(flat, offs, s)
    qm.sync()
    assert qm.position_count() == launches * per_launch
    all_want = np.tile(want, (launches * copies, 1))
    assert_same(qm.positions(), all_want, "after the growth")
    assert_same(qm.positions(49_000, 1_000), all_want[49_000:50_000], "across the carried / new boundary")
    qm.reset()  # the grown buffer is cleared over its used prefix
    one_flat, one_offs = flatten_reads(reads)
    qm.map_reads(one_flat, one_offs, seeds)
    assert qm.position_count() == len(reads)
    assert_same(qm.positions(), want, "after the reset")


@pytest.mark.parametrize("name", ["nested", "repeat", "half_sited"])
def test_serial_coverage_instances_give_the_cooperative_kernels_records(monkeypatch, name):
    """GMX_NO_COOP=1: every general task goes through the one-lane instances (gmx_cover_task) instead of the 16-lane cooperative
    kernel, which reduces the minimum and the count over lanes: the same records, the oracle's."""
    prg, k, reads, seeds, want, _ = case(name)
    monkeypatch.setenv("GMX_NO_COOP", "1")
    got, _, _ = record(Index(prg, k), reads, seeds)
    assert_same(got, want, name)


def test_recording_off_leaves_nothing_and_changes_nothing():
    prg, k, reads, seeds, _, _ = case("flat")
    ix = Index(prg, k)
    flat, offs = flatten_reads(reads)
    off = Quasimapper(ix)
    off.record_outcomes(True)
    off.map_reads(flat, offs, seeds)
    assert off.position_count() == 0 and off.positions().shape == (0, 4)
    a = off.coverage()
    _, out, on = record(ix, reads, seeds)
    b = on.coverage()
    assert (a.raw_allele_sum == b.raw_allele_sum).all() and (a.raw_per_base == b.raw_per_base).all()
    assert (a.raw_grouped == b.raw_grouped).all() and a.stats.as_dict() == b.stats.as_dict()
    assert off.outcomes().tolist() == out.tolist()
    on.record_positions(False)  # switched off again: later calls append nothing
    on.map_reads(flat, offs, seeds)
    assert on.position_count() == len(reads) and on.outcome_count() == 2 * len(reads)
    with pytest.raises(ValueError):
        on.positions(0, len(reads) + 1)


def test_forward_only_engine_leaves_the_reverse_halves_zero():
    prg, k, reads, seeds, want, _ = case("flat")
    got, out, _ = record(Index(prg, k), reads, seeds, forward_only=True)
    assert_same(got[:, :2], want[:, :2], "forward halves")
    assert not got[:, 2:].any()


# ---- capacity tiers, the grouped log ---------------------------------------------------------------------------------
def test_every_tier_leaves_the_records_of_the_default_capacities():
    """300 tandem copies (the case of test_read_outcomes' tier test): default pools against small ones, which send the tasks through
    the split search, the one-lane slot and the heap-backed tier. The same records, the oracle's, n == 300 among them."""
    prg, unit, site_at, alt = tandem_prg(300, 60, 5)
    reads = tandem_reads(unit, site_at, alt, 100, 6)
    reads += [np.asarray(r[:40]) for r in reads[:3]] + [np.asarray([int(x) for x in prg[3:33]], dtype=np.uint8)]
    ix = Index(prg, 8)
    seeds = default_seeds(len(reads))
    want, _ = oracle_records(prg, 8, reads, seeds)
    assert (want[:, [1, 3]] == 300).any()
    big, _, qm = record(ix, reads, seeds)
    counts = qm.queue_counts()
    assert counts["big_mapped"] + counts["inst_mapped"] + counts["cover_overflow"] > 0 and counts["huge_search"] + counts["huge_cover"] == 0
    assert_same(big, want, "default pools")
    small, _, qm2 = record(ix, reads, seeds, max_states=64, max_path_nodes=128)
    counts2 = qm2.queue_counts()
    assert counts2["overflow_probe"] + counts2["overflow_extend"] >= 4, counts2
    assert counts2["overflow_split"] >= 4, counts2
    assert counts2["huge_search"] >= 4, counts2
    assert_same(small, want, "small pools")


def test_a_tiny_grouped_log_replays_and_leaves_the_same_records():
    from gramtools_amd.synth import mixed_variant_prg, simulate_haplotype_reads
    ref = random_ref(3000, 5)
    prg, sites = mixed_variant_prg(ref, 60, 6, max_alleles=12)
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_haplotype_reads(ref, sites, 600, 40, 80, 7)]
    ix = Index(prg, 6)
    seeds = default_seeds(len(reads))
    want, _ = oracle_records(prg, 6, reads, seeds)
    roomy, _, _ = record(ix, reads, seeds)
    assert_same(roomy, want, "roomy log")
    tiny, _, qm = record(ix, reads, seeds, chunk=150, log_cap_words=64)
    assert qm.queue_counts()["log_replays"] > 0
    assert_same(tiny, roomy, "tiny log")


# ---- engine groups ---------------------------------------------------------------------------------------------------
def test_a_group_puts_its_engines_records_together_in_read_order():
    from gramtools_amd import QuasimapperGroup
    prg, k, reads, _, _, _ = case("flat")
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    want, _, _ = record(ix, reads, seeds)
    for devices in ([0, 0], [0, 0, 0]):
        grp = QuasimapperGroup(ix, devices)
        assert grp.position_count() == 0
        grp.record_positions(True)
        cuts = [0, 101, 350, len(reads)]
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            flat, offs = flatten_reads(reads[lo:hi])
            if j == 1:
                pk = pack_reads(flat, offs, pinned=True)
                grp.map_reads_packed(pk, seeds[lo:hi])
            else:
                grp.map_reads(flat, offs, seeds[lo:hi])
        assert grp.position_count() == len(reads) and grp.outcome_count() == 0
        assert_same(grp.positions(), want, devices)
        assert_same(grp.positions(97, 300), want[97:397], "a sub-range")
        grp.allreduce()
        assert_same(grp.positions(), want, "after the exchange")
        for i in range(len(devices)):
            assert grp.lib.gmx_engine_reset(C.c_void_p(grp.lib.gmx_group_engine(grp.h, i))) == 0
        assert grp.position_count() == 0
        flat, offs = flatten_reads(reads[200:])
        grp.map_reads(flat, offs, seeds[200:])
        assert_same(grp.positions(), want[200:], "after the members' reset")
        pk.close()
        grp.close()


# ---- gram genotype --read_positions ----------------------------------------------------------------------------------
COV_FILES = ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")


def parse_positions_file(data: bytes):
    """read_positions.bin: "GMXP", uint32 version 1, uint64 read count (little-endian), then four uint32 per read."""
    magic, version, n = struct.unpack_from("<4sIQ", data, 0)
    assert magic == b"GMXP" and version == 1 and len(data) == 16 + 16 * n, (magic, version, n, len(data))
    return np.frombuffer(data, dtype="<u4", offset=16).reshape(n, 4)


@pytest.fixture(scope="module")
def cli_sample(tmp_path_factory):
    """About 7 000 ragged reads of up to 60 bases with Ns in the forms `gram` reads, the run without the flag, and the records the
    engine itself gives for these reads."""
    from bam_common import bam_bytes, record as bam_record, reverse_complement
    from ingest_formats_common import gram
    from test_ingest import bgzf
    d = tmp_path_factory.mktemp("positions_cli")
    rng = np.random.default_rng(3)
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    (d / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    reads = simulate_snp_reads(ref, pos, alts, n_alts, 7300, 60, 6)
    txt = ["".join("ACGT"[b - 1] for b in r) for r in reads]
    txt = [t[:int(rng.integers(20, 61))] for t in txt]
    for i in range(0, len(txt), 97):
        txt[i] = txt[i][:7] + "N" + txt[i][8:]
    fq = "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(txt)).encode()
    (d / "s.fq").write_bytes(fq)
    (d / "s.bgzf.fq.gz").write_bytes(bgzf(fq, block=9000))
    recs = []
    for i, s in enumerate(txt):
        back = i % 3 == 1
        recs.append(bam_record(reverse_complement(s) if back else s, flag=0x10 if back else 0, name=f"r{i}", qual=bytes([40]) * len(s)))
    (d / "s.bam").write_bytes(bgzf(bam_bytes(recs, [("chr1", 3000)], "@HD\tVN:1.6\n"), block=9000))

    def run(name, reads_file, env=None, extra=()):
        out = d / name
        r = gram("genotype", "--gram_dir", str(d), "--reads", str(d / reads_file), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", "6",
                 "--genotype_dir", str(out), "--seed", "1234", *extra, env=env or {})
        assert r.returncode == 0, (name, r.stdout)
        return out, r.stdout

    plain_out, _ = run("noflag", "s.fq", {"GMX_HOST_FASTQ": "1"})
    code = {c: v for c, v in zip("ACGT", (1, 2, 3, 4))}
    enc = [np.asarray([code.get(c, 0) for c in s], dtype=np.uint8) for s in txt]
    want, _, _ = record(Index(prg, 6), enc, master_seeds(1234, [len(enc)]))
    return dict(run=run, cov=[(plain_out / "coverage" / f).read_bytes() for f in COV_FILES], want=want, noflag=plain_out)


CLI_FORMS = [("plain-one-thread", "s.fq", {}, ["--max_threads", "1"]),
             ("plain-host-parser", "s.fq", {"GMX_HOST_FASTQ": "1"}, []),
             ("bgzf", "s.bgzf.fq.gz", {}, []),
             ("bam", "s.bam", {}, []),
             ("two-engines", "s.fq", {"GMX_TEXT_CHUNK": "30000"}, ["--devices", "0,0"]),
             ("takeover", "s.bgzf.fq.gz", {"GMX_INGEST_MEMBERS": "20", "GMX_INGEST_TEST_FAIL_CHUNK": "2", "GMX_FASTQ_BLOCK": "200000"}, [])]


@pytest.mark.parametrize("name,reads_file,env,extra", CLI_FORMS, ids=[f[0] for f in CLI_FORMS])
def test_gram_read_positions_on_every_route(cli_sample, name, reads_file, env, extra):
    """Every form of the sample gives the SAME read_positions.bin — the records the engine gives for these reads in file order —,
    json counts that add up, and the three coverage files of a run without the flag."""
    out, stdout = cli_sample["run"](name, reads_file, env, ["--read_positions", *extra])
    if name.startswith("takeover"):
        assert "the host reader takes over" in stdout and "gave up after 0 reads" not in stdout, stdout
    got = parse_positions_file((out / "read_positions.bin").read_bytes())
    assert got.shape == (7300, 4)
    assert_same(got.astype(np.uint32), cli_sample["want"], name)
    n = np.concatenate([got[:, 1], got[:, 3]])
    js = json.loads((out / "read_positions.json").read_text())
    assert js["reads"] == 7300
    assert js["tasks_mapped"] == int((n > 0).sum()) > 1000
    assert js["tasks_one_instance"] == int((n == 1).sum()) and js["tasks_several_instances"] == int((n > 1).sum())
    assert js["tasks_one_instance"] + js["tasks_several_instances"] == js["tasks_mapped"]
    hist = js["instances_histogram"]
    assert [hist[b] for b in ("1", "2", "3-10", "11-100", "above_100")] == [int(((n >= lo) & (n <= hi)).sum()) for lo, hi in
                                                                              ((1, 1), (2, 2), (3, 10), (11, 100), (101, 2 ** 32))]
    assert sum(hist.values()) == js["tasks_mapped"]
    counters = [int(l.rsplit(":", 1)[1]) for l in stdout.splitlines() if l.startswith("Count ")]
    assert len(counters) == 5 and counters[4] == js["tasks_mapped"]  # (exact_mapped)
    assert [(out / "coverage" / f).read_bytes() for f in COV_FILES] == cli_sample["cov"]
    assert not (cli_sample["noflag"] / "read_positions.bin").exists() and not (cli_sample["noflag"] / "read_positions.json").exists()
    assert not (out / "read_outcomes.bin").exists()


def test_gram_read_positions_beside_the_other_recordings(cli_sample):
    """--read_positions with --read_outcomes, --strand_coverage and --strand_bias: the same records, the others' files present."""
    out, _ = cli_sample["run"]("combined", "s.fq", {}, ["--read_positions", "--read_outcomes", "--strand_coverage", "--strand_bias"])
    got = parse_positions_file((out / "read_positions.bin").read_bytes())
    assert_same(got.astype(np.uint32), cli_sample["want"], "combined")
    assert (out / "read_outcomes.bin").exists()
    assert [(out / "coverage" / f).read_bytes() for f in COV_FILES] == cli_sample["cov"]

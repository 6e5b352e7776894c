"""Per-site ambiguity counts (gmx_engine_record_site_ambiguity, include/gmx.h): two uint32 per site — drawn, the
ambiguous tasks whose drawn class recorded at the site, and passed, the candidate placements at the site of ambiguous tasks that
ended mapped without recording a class. The expectation comes from the oracle alone (site_ambiguity_common.py). A task counts
exactly once on every routine that finishes it: the cooperative kernel, the serial instances, the tiers, the log replay, both
workspaces, every feed, engine groups and `gram genotype --site_ambiguity`; and the recording changes nothing else."""
import ctypes as C
import functools
import gzip
import json

import numpy as np
import pytest

from common import canonical_cov, flatten_reads
from gramtools_amd import GmxError, Index, Quasimapper, QuasimapperGroup, master_seeds, pack_reads
from gramtools_amd.synth import mixed_variant_prg, random_ref, simulate_haplotype_reads
from max_candidates_common import case, describe_tasks
from site_ambiguity_common import expect_from, expectation
from test_many_instances import tandem_prg, tandem_reads
from test_max_candidates import COV_FILES, cli, files  # noqa: F401  (cli: a fixture)
from test_read_outcomes import FEEDS, run_feed
from test_site_ambiguity_host import strip_json, strip_vcf

pytestmark = pytest.mark.gpu

GMX_EINVAL = -1


@functools.lru_cache(maxsize=None)
def index_of(name):
    prg, k, _, _ = case(name)
    return Index(prg, k)


def run(ix, reads, seeds, limit, on=True, feed="bytes", chunk=0, strands=False, **kw):
    """(drawn, passed, canonical coverage, outcome bytes, position records, engine) of `reads` under `limit`; on=False: recording
    off, drawn and passed None."""
    qm = Quasimapper(ix, **kw)
    qm.record_outcomes(True)
    qm.record_positions(True)
    if strands:
        qm.record_strands(True)
    if on:
        qm.record_site_ambiguity(True)
    assert bool(qm.lib.gmx_engine_site_ambiguity(qm.h)) == on
    if limit:
        qm.set_max_candidates(limit)
    run_feed(qm, reads, seeds, feed, chunk)
    drawn, passed = qm.site_ambiguity() if on else (None, None)
    return drawn, passed, canonical_cov(qm.coverage()), qm.outcomes(), qm.positions(), qm


def same_counts(got, want, note=""):
    for which, g, w in (("drawn", got[0], want[0]), ("passed", got[1], want[1])):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.uint32 and g.shape == w.shape, (note, which, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (note, which, [(int(s), int(g[s]), int(w[s])) for s in bad[:10]])


def same_rest(a, b, note=""):
    """coverage, outcome bytes and position records of two runs"""
    assert a[2] == b[2], (note, "coverage")
    assert a[3].tolist() == b[3].tolist(), (note, "outcomes")
    assert a[4].tolist() == b[4].tolist(), (note, "positions")


@functools.lru_cache(maxsize=None)
def engine_run(name, limit, on=True):
    _, _, reads, seeds = case(name)
    return run(index_of(name), reads, seeds, limit, on)[:5]


# ---- 1. the cases against the expectation ----------------------------------------------------------------------------
CASE_LIMITS = [("ladder", L) for L in (0, 1, 2, 5)] + [("nested_ladder", L) for L in (0, 1, 3)] + [("half_sited", L) for L in (0, 9, 10)]


@pytest.mark.parametrize("name,limit", CASE_LIMITS, ids=[f"{n}-{L}" for n, L in CASE_LIMITS])
def test_cases_against_the_oracles_expectation(name, limit):
    got = engine_run(name, limit)
    same_counts(got, expectation(name, limit), (name, limit))
    same_rest(got, engine_run(name, limit, False), (name, limit))  # the recording changes nothing else
    if limit == 1:
        assert not got[0].any() and got[1].any()


# ---- 2. two identities that need no oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "nested_ladder", "half_sited"])
def test_drawn_is_the_grouped_coverage_the_limit_one_run_lacks(name):
    """Per site: a task adds one grouped count where its class records; limit 1 keeps exactly the tasks that are not ambiguous."""
    free, one = engine_run(name, 0), engine_run(name, 1)
    per_site = lambda run_: np.asarray([sum(site.values()) for site in run_[2]["grouped"]], dtype=np.int64)
    assert (per_site(free) - per_site(one)).tolist() == free[0].tolist()
    assert free[0].any()


def test_half_sited_every_ambiguous_task_is_drawn_or_passed_over():
    """Every ambiguous task of half_sited has five single-site classes, one per sited copy. With the limit at 1 it adds 1 to `passed`
    of each of the five sites. With the limit off it either falls on the non-variant instances — the same five placements — or
    draws ONE class and adds 1 to `drawn` of that one site. So for every site s: passed1[s] == passed0[s] + sum(drawn0) (the tasks).
    (Per site, drawn0[s] + passed0[s] == passed1[s] cannot hold under these semantics: a task that drew records at one site of the
    five it is a candidate at. Oracle and engine: drawn0 + passed0 = [35, 33, 30, 32, 33] against passed1 = [55] * 5.)"""
    free, one = engine_run("half_sited", 0), engine_run("half_sited", 1)
    print("drawn0", free[0].tolist(), "passed0", free[1].tolist(), "passed1", one[1].tolist())
    assert free[0].any() and free[1].any()
    assert (free[1].astype(np.int64) + int(free[0].sum())).tolist() == one[1].tolist()
    assert len(set(free[1].tolist())) == 1 and not one[0].any()


# ---- 3. routes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("ladder", 0), ("ladder", 2), ("nested_ladder", 0), ("half_sited", 0), ("half_sited", 9)])
def test_serial_coverage_instances_count_what_the_cooperative_kernel_counts(monkeypatch, name, limit):
    """GMX_NO_COOP=1: every general task goes through gmx_cover_task on one lane instead of the 16-lane kernel."""
    _, _, reads, seeds = case(name)
    coop = engine_run(name, limit)
    monkeypatch.setenv("GMX_NO_COOP", "1")
    serial = run(index_of(name), reads, seeds, limit)
    same_counts(serial, expectation(name, limit), (name, limit, "serial"))
    same_counts(serial, coop, "serial against cooperative")
    same_rest(serial, coop, "serial against cooperative")


@pytest.mark.parametrize("twin", ["0", "1"])
@pytest.mark.parametrize("name", ["ladder", "nested_ladder"])
def test_every_feed_and_both_workspaces(monkeypatch, twin, name):
    monkeypatch.setenv("GMX_TWIN", twin)
    _, _, reads, seeds = case(name)
    want = expectation(name, 2)
    for feed in FEEDS:
        got = run(index_of(name), reads, seeds, 2, feed=feed, chunk=97)
        assert bool(got[5].lib.gmx_engine_second_stream(got[5].h)) == (twin == "1")
        same_counts(got, want, (name, feed, twin))


@functools.lru_cache(maxsize=None)
def tier_case():
    prg, unit, site_at, alt = tandem_prg(300, 60, 5)
    reads = tandem_reads(unit, site_at, alt, 100, 6)
    reads += [np.asarray(r[:40]) for r in reads[:3]] + [np.asarray([int(x) for x in prg[3:33]], dtype=np.uint8)]
    seeds = master_seeds(7, [len(reads)])
    return prg, reads, seeds


@pytest.mark.parametrize("limit", [0, 100])
def test_a_task_counts_once_whichever_tier_finishes_it(limit):
    """300 tandem copies: default pools against small ones, which send the tasks through the split search, the one-lane slot and the
    heap-backed tier. A task turned away by one tier and finished by the next must not have counted on its first pass."""
    prg, reads, seeds = tier_case()
    ix = Index(prg, 8)
    big = run(ix, reads, seeds, limit)
    counts = big[5].queue_counts()
    assert counts["huge_search"] + counts["huge_cover"] == 0
    small = run(ix, reads, seeds, limit, max_states=64, max_path_nodes=128)
    assert small[5].queue_counts()["huge_search"] >= 4
    same_counts(small, big, ("small pools against default pools", limit))
    same_rest(small, big, ("tiers", limit))
    assert (big[1] if limit else big[0]).any()
    if limit:
        assert int(big[1].max()) >= 4  # at least four tasks of nearly 300 candidates were left out: every copy's site was passed over


def test_a_tiny_grouped_log_replays_without_counting_twice():
    ref = random_ref(3000, 5)
    prg, sites = mixed_variant_prg(ref, 60, 6, max_alleles=12)
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_haplotype_reads(ref, sites, 600, 40, 80, 7)]
    seeds = master_seeds(7, [len(reads)])
    ix = Index(prg, 6)
    tasks = describe_tasks(prg, 6, reads, seeds)
    for limit in (0, 1):
        roomy = run(ix, reads, seeds, limit)
        tiny = run(ix, reads, seeds, limit, chunk=150, log_cap_words=64)
        assert tiny[5].queue_counts()["log_replays"] > 0
        same_counts(tiny, roomy, ("tiny log against roomy log", limit))
        assert tiny[2] == roomy[2]
        same_counts(roomy, expect_from(prg, 6, tasks, limit), ("roomy log", limit))


# ---- 4. switching ----------------------------------------------------------------------------------------------------
def test_switching_only_while_nothing_is_recorded_and_the_recording_survives_a_reset():
    _, _, reads, seeds = case("nested_ladder")
    ix = index_of("nested_ladder")
    qm = Quasimapper(ix)
    lib = qm.lib
    assert lib.gmx_engine_site_ambiguity(qm.h) == 0
    none = np.zeros(ix.n_sites, dtype=np.uint32)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.gmx_coverage_fetch_site_ambiguity(qm.h, u32(none), u32(none), ix.n_sites) == GMX_EINVAL  # recording is off
    with pytest.raises(GmxError):
        qm.site_ambiguity()
    qm.record_site_ambiguity(True)
    qm.record_site_ambiguity(False)
    qm.record_site_ambiguity(True)
    assert lib.gmx_engine_site_ambiguity(qm.h) == 1
    assert lib.gmx_coverage_fetch_site_ambiguity(qm.h, u32(none), u32(none), ix.n_sites + 1) == GMX_EINVAL and b"n_sites" in lib.gmx_last_error()
    assert not qm.site_ambiguity()[0].any() and not qm.site_ambiguity()[1].any()
    run_feed(qm, reads, seeds, "bytes")
    same_counts(qm.site_ambiguity(), expectation("nested_ladder", 0), "first job")
    assert lib.gmx_engine_record_site_ambiguity(qm.h, 0) == GMX_EINVAL and b"gmx_engine_reset" in lib.gmx_last_error()
    with pytest.raises(GmxError):
        qm.record_site_ambiguity(False)
    assert lib.gmx_engine_site_ambiguity(qm.h) == 1
    same_counts(qm.site_ambiguity(), expectation("nested_ladder", 0), "a refused switch leaves the counts")
    qm.reset()
    assert lib.gmx_engine_site_ambiguity(qm.h) == 1  # the recording survives the reset, the counts do not
    assert not qm.site_ambiguity()[0].any() and not qm.site_ambiguity()[1].any()
    qm.set_max_candidates(3)
    run_feed(qm, reads, seeds, "bytes")
    same_counts(qm.site_ambiguity(), expectation("nested_ladder", 3), "second job")
    qm.reset()
    qm.record_site_ambiguity(False)  # allowed after a reset
    run_feed(qm, reads, seeds, "bytes")
    assert canonical_cov(qm.coverage()) == engine_run("nested_ladder", 3, False)[2]


@pytest.mark.parametrize("name,limit", [("ladder", 2), ("half_sited", 0)])
def test_combined_with_per_strand_recording(name, limit):
    _, _, reads, seeds = case(name)
    both = run(index_of(name), reads, seeds, limit, strands=True)
    same_counts(both, expectation(name, limit), "with record_strands")
    same_rest(both, engine_run(name, limit), "with record_strands")
    qm = both[5]
    fwd, rev = qm.coverage(strand=0), qm.coverage(strand=1)
    total = qm.coverage()
    assert ((fwd.raw_allele_sum + rev.raw_allele_sum) == total.raw_allele_sum).all() and fwd.raw_allele_sum.any() and rev.raw_allele_sum.any()
    assert ((fwd.raw_per_base + rev.raw_per_base) == total.raw_per_base).all()
    assert ((fwd.raw_grouped + rev.raw_grouped) == total.raw_grouped).all()


# ---- 5. engine groups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two", "three"])
def test_a_group_sums_to_the_single_engine(devices):
    _, _, reads, seeds = case("ladder")
    ix = index_of("ladder")
    single = engine_run("ladder", 2)
    grp = QuasimapperGroup(ix, devices)
    grp.record_site_ambiguity(True)
    grp.set_max_candidates(2)
    members = [C.c_void_p(grp.lib.gmx_group_engine(grp.h, i)) for i in range(len(devices))]
    assert [grp.lib.gmx_engine_site_ambiguity(m) for m in members] == [1] * len(devices)
    cuts = [0, 101, 250, len(reads)]
    for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        flat, offs = flatten_reads(reads[lo:hi])
        if j == 1:
            pk = pack_reads(flat, offs, pinned=True)
            grp.map_reads_packed(pk, seeds[lo:hi])
        else:
            grp.map_reads(flat, offs, seeds[lo:hi])
    grp.allreduce()
    for member in range(len(devices)):
        same_counts(grp.site_ambiguity(member), single, (devices, member))
    assert canonical_cov(grp.coverage()) == single[2]
    # its members have recorded: none is changed
    assert grp.lib.gmx_group_record_site_ambiguity(grp.h, 0) == GMX_EINVAL
    assert [grp.lib.gmx_engine_site_ambiguity(m) for m in members] == [1] * len(devices)
    pk.close()
    grp.close()


def test_a_group_whose_members_disagree_does_not_exchange():
    ix = index_of("ladder")
    _, _, reads, seeds = case("ladder")
    grp = QuasimapperGroup(ix, [0, 0])
    grp.record_site_ambiguity(True)
    member = C.c_void_p(grp.lib.gmx_group_engine(grp.h, 1))
    assert grp.lib.gmx_engine_record_site_ambiguity(member, 0) == 0  # one member switched off behind the group's back
    flat, offs = flatten_reads(reads[:50])
    grp.map_reads(flat, offs, seeds[:50])
    assert grp.lib.gmx_group_allreduce(grp.h) == GMX_EINVAL and b"gmx_group_record_site_ambiguity" in grp.lib.gmx_last_error()
    grp.close()


# ---- 6. gram genotype --site_ambiguity -------------------------------------------------------------------------------
def amb_files(out):
    js = json.loads((out / "coverage" / "site_ambiguity.json").read_text())
    assert list(js) == ["site_ambiguity"] and list(js["site_ambiguity"]) == ["drawn", "passed_over"]
    return js["site_ambiguity"]["drawn"], js["site_ambiguity"]["passed_over"], json.loads((out / "site_ambiguity.json").read_text())


def gram_expectation(seed, limit):
    prg, k, reads, _ = case("ladder")
    return expect_from(prg, k, describe_tasks(prg, k, reads, master_seeds(seed, [len(reads)])), limit)


def all_files(out):
    return sorted(str(p.relative_to(out)) for p in out.rglob("*") if p.is_file())


def test_gram_writes_the_counts_and_the_calls_carry_them(cli):
    out, _ = cli("amb-seed1", seed="1", extra=["--site_ambiguity"])
    drawn, passed, summary = amb_files(out)
    want = gram_expectation(1, 0)
    assert drawn == want[0].tolist() and passed == want[1].tolist() and any(drawn)
    assert summary == {"sites": len(drawn), "sites_drawn": sum(1 for x in drawn if x), "sites_passed_over": sum(1 for x in passed if x),
                       "drawn": sum(drawn), "passed_over": sum(passed)}
    j = json.loads((out / "genotype" / "genotyped.json").read_text())
    assert {"AMB_DRAWN", "AMB_PASSED"} <= set(j["Site_Fields"]) and len(j["Sites"]) == len(drawn)
    for s, site in enumerate(j["Sites"]):
        null = site["GT"][0][0] is None
        assert site["AMB_DRAWN"] == ([None] if null else [drawn[s]]) and site["AMB_PASSED"] == ([None] if null else [passed[s]]), s
    assert any(site["GT"][0][0] is not None and site["AMB_DRAWN"][0] for site in j["Sites"])
    vcf = gzip.decompress((out / "genotype" / "genotyped.vcf.gz").read_bytes()).decode()
    recs = [l.split("\t") for l in vcf.splitlines() if not l.startswith("#")]
    assert len(recs) == len(drawn)  # a flat PRG: every site is a level-1 site
    for s, r in enumerate(recs):
        f = dict(zip(r[8].split(":"), r[9].split(":")))
        assert r[8].endswith(":AMB_DRAWN:AMB_PASSED")
        assert (f["AMB_DRAWN"], f["AMB_PASSED"]) == ((".", ".") if f["GT"] == "." else (str(drawn[s]), str(passed[s]))), s
    # without the flag: no new file, and every other file is what the run with the flag wrote, the two fields aside
    plain, _ = cli("off-seed1", seed="1")
    assert all_files(out) == sorted(all_files(plain) + ["coverage/site_ambiguity.json", "site_ambiguity.json"])
    assert files(plain) == files(out)
    assert (plain / "genotype" / "personalised_reference.fasta").read_bytes() == (out / "genotype" / "personalised_reference.fasta").read_bytes()
    plain_json = (plain / "genotype" / "genotyped.json").read_text()
    assert "AMB_" not in plain_json and strip_json((out / "genotype" / "genotyped.json").read_text()) == plain_json
    plain_vcf = gzip.decompress((plain / "genotype" / "genotyped.vcf.gz").read_bytes()).decode()
    assert "AMB_" not in plain_vcf and strip_vcf(vcf) == plain_vcf


def test_gram_two_engines_write_the_same_files(cli):
    ref, _ = cli("amb-seed1", seed="1", extra=["--site_ambiguity"])
    out, _ = cli("amb-two-engines", seed="1", extra=["--site_ambiguity", "--devices", "0,0"], env={"GMX_TEXT_CHUNK": "6000"})
    assert amb_files(out) == amb_files(ref) and files(out) == files(ref)
    for f in ("genotyped.json", "genotyped.vcf.gz"):
        assert (out / "genotype" / f).read_bytes() == (ref / "genotype" / f).read_bytes(), f


def test_gram_limit_one_passes_over_the_same_placements_whatever_the_seed(cli):
    a, _ = cli("amb-limit1-seed1", seed="1", extra=["--site_ambiguity", "--max_candidates", "1"])
    b, _ = cli("amb-limit1-seed2", seed="2", extra=["--site_ambiguity", "--max_candidates", "1", "--strand_coverage", "--strand_bias",
                                                    "--read_outcomes", "--read_positions"])
    da, pa, _ = amb_files(a)
    db, pb, _ = amb_files(b)
    assert pa == pb == gram_expectation(1, 1)[1].tolist() and any(pa)
    assert not any(da) and not any(db)
    vcf = gzip.decompress((b / "genotype" / "genotyped.vcf.gz").read_bytes()).decode()
    recs = [l.split("\t") for l in vcf.splitlines() if not l.startswith("#")]
    assert all(r[8].endswith(":COV_FWD:COV_REV:SB:AMB_DRAWN:AMB_PASSED") for r in recs)  # behind the strand fields

"""The limit on a selection's candidates (gmx_engine_set_max_candidates, include/gmx.h): a task with a class whose
draw would range over more than L candidates is left out — no draw, no coverage, nothing in the grouped log — but stays an exactly
mapped task: the five counters are those of the limit-off run, its outcome code stays 3 with bit 6 / 7 instead of the multi bit,
and its position record keeps n with pos the smallest position among all its instances. The expectation comes from the oracle
alone (max_candidates_common.py). Compared on every routine that draws: the cooperative kernel, the serial instances, the tiers,
the log replay, the workspaces, the feeds, engine groups and `gram genotype --max_candidates`."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from common import canonical_cov, flatten_reads
from gramtools_amd import GmxError, Index, Quasimapper, QuasimapperGroup, master_seeds, pack_reads
from gramtools_amd.synth import mixed_variant_prg, random_ref, simulate_haplotype_reads
from max_candidates_common import (allele_sum_total, case, describe_tasks, described, expect_from, expectation, total_of,
                                   without_stats)
from test_many_instances import tandem_prg, tandem_reads
from test_read_outcomes import FEEDS, run_feed
from test_read_positions import assert_same

pytestmark = pytest.mark.gpu

GMX_EINVAL = -1


@functools.lru_cache(maxsize=None)
def index_of(name):
    prg, k, _, _ = case(name)
    return Index(prg, k)


def run(ix, reads, seeds, limit, feed="bytes", chunk=0, **kw):
    """(canonical coverage, outcome bytes, position records, engine) of `reads` under `limit` (None: the engine is never told)."""
    qm = Quasimapper(ix, **kw)
    qm.record_outcomes(True)
    qm.record_positions(True)
    if limit is not None:
        qm.set_max_candidates(limit)
        assert qm.max_candidates == limit
    run_feed(qm, reads, seeds, feed, chunk)
    return canonical_cov(qm.coverage()), qm.outcomes(), qm.positions(), qm


@functools.lru_cache(maxsize=None)
def limit_off(name):
    """The engine's own run of a case with the limit off: (canonical coverage, outcome bytes)."""
    _, _, reads, seeds = case(name)
    cov, out, _, _ = run(index_of(name), reads, seeds, None)
    return cov, out


def check(got, want, note=""):
    cov, out, pos = got[:3]
    for key in want["cov"]:
        assert cov[key] == want["cov"][key], (note, key)
    bad = np.flatnonzero(out != want["bytes"])
    assert bad.size == 0, (note, [(int(i), hex(int(out[i])), hex(int(want["bytes"][i]))) for i in bad[:10]])
    assert_same(pos, want["positions"], note)


# ---- 1. the cases against the expectation ----------------------------------------------------------------------------
CASE_LIMITS = [("ladder", L) for L in (1, 2, 3, 5, 9)] + [("nested_ladder", L) for L in (1, 2, 3, 5)] + [("half_sited", L) for L in (1, 9, 10)]


@pytest.mark.parametrize("name,limit", CASE_LIMITS, ids=[f"{n}-{L}" for n, L in CASE_LIMITS])
def test_cases_against_the_oracles_expectation(name, limit):
    _, _, reads, seeds = case(name)
    want = expectation(name, limit)
    got = run(index_of(name), reads, seeds, limit)
    check(got, want, (name, limit))
    off_cov, off_out = limit_off(name)
    assert got[0]["stats"] == off_cov["stats"]  # still exactly mapped tasks: the five counters do not move
    assert ((got[1] & 0x0F) == (off_out & 0x0F)).all()  # ... nor do the task codes
    left = int(np.unpackbits(got[1] & 0xC0).sum())
    assert left == len(want["left_out"])
    assert not (got[1] & 0xC0 & ((got[1] & 0x30) << 2)).any()  # a left-out task did not draw: never both bits
    if want["left_out"]:
        assert allele_sum_total(got[0]) < allele_sum_total(off_cov)


def test_the_limit_off_run_is_the_expectation_without_a_limit():
    for name in ("ladder", "nested_ladder", "half_sited"):
        cov, out = limit_off(name)
        want = expectation(name, 0)
        assert without_stats(cov) == want["cov"] and out.tolist() == want["bytes"].tolist(), name


# ---- 2. no draw, no dependence on the seeds --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "nested_ladder"])
def test_limit_one_makes_the_coverage_independent_of_seeds_and_rng_mode(name):
    _, _, reads, seeds = case(name)
    other = master_seeds(12345, [len(reads)])
    assert (other != seeds).any()
    want = expectation(name, 1)["cov"]
    for s in (seeds, other):
        for mode in (0, 1):
            cov, _, _, _ = run(index_of(name), reads, s, 1, rng_mode=mode)
            assert without_stats(cov) == want, (name, mode)
    a, _, _, _ = run(index_of(name), reads, seeds, 0)
    b, _, _, _ = run(index_of(name), reads, other, 0)
    assert without_stats(a) != without_stats(b)  # with the limit off the seeds decide: the case has something to filter


# ---- 3. routes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,limit", [("ladder", 2), ("nested_ladder", 2), ("half_sited", 9), ("half_sited", 10)])
def test_serial_coverage_instances_give_what_the_cooperative_kernel_gives(monkeypatch, name, limit):
    """GMX_NO_COOP=1: every general task goes through gmx_cover_task on one lane instead of the 16-lane kernel."""
    _, _, reads, seeds = case(name)
    coop = run(index_of(name), reads, seeds, limit)
    monkeypatch.setenv("GMX_NO_COOP", "1")
    serial = run(index_of(name), reads, seeds, limit)
    check(serial, expectation(name, limit), (name, limit, "serial"))
    assert serial[0] == coop[0] and serial[1].tolist() == coop[1].tolist()
    assert_same(serial[2], coop[2], "serial against cooperative")


@pytest.mark.parametrize("twin", ["0", "1"])
@pytest.mark.parametrize("name", ["ladder", "nested_ladder"])
def test_every_feed_and_both_workspaces(monkeypatch, twin, name):
    monkeypatch.setenv("GMX_TWIN", twin)
    _, _, reads, seeds = case(name)
    want = expectation(name, 2)
    for feed in FEEDS:
        for chunk in (0, 97):
            got = run(index_of(name), reads, seeds, 2, feed=feed, chunk=chunk)
            assert bool(got[3].lib.gmx_engine_second_stream(got[3].h)) == (twin == "1")
            check(got, want, (name, feed, chunk, twin))


@functools.lru_cache(maxsize=None)
def tier_case():
    prg, unit, site_at, alt = tandem_prg(300, 60, 5)
    reads = tandem_reads(unit, site_at, alt, 100, 6)
    reads += [np.asarray(r[:40]) for r in reads[:3]] + [np.asarray([int(x) for x in prg[3:33]], dtype=np.uint8)]
    seeds = master_seeds(7, [len(reads)])
    return prg, reads, seeds, describe_tasks(prg, 8, reads, seeds)


@pytest.mark.parametrize("limit", [100, 300])
def test_every_tier_decides_alike(limit):
    """300 tandem copies (test_read_outcomes' tier case): default pools against small ones, which send the tasks through the split
    search, the one-lane slot and the heap-backed tier, where they meet the same decision: nearly 300 candidates against 100, or against 300."""
    prg, reads, seeds, tasks = tier_case()
    assert 290 <= max(total_of(d[6]) for d in tasks) <= 300  # (the copies at the array's ends are out of a 100-base read's reach)
    want = expect_from(prg, 8, tasks, limit)
    assert bool(want["left_out"]) == (limit == 100) and (limit == 300 or len(want["left_out"]) >= 4)
    ix = Index(prg, 8)
    big = run(ix, reads, seeds, limit)
    counts = big[3].queue_counts()
    assert counts["big_mapped"] + counts["inst_mapped"] + counts["cover_overflow"] > 0 and counts["huge_search"] + counts["huge_cover"] == 0
    check(big, want, ("default pools", limit))
    small = run(ix, reads, seeds, limit, max_states=64, max_path_nodes=128)
    assert small[3].queue_counts()["huge_search"] >= 4
    check(small, want, ("small pools", limit))
    assert small[0] == big[0]


# ---- 4. a site on the grouped log ------------------------------------------------------------------------------------
def test_a_tiny_grouped_log_replays_under_the_same_limit():
    ref = random_ref(3000, 5)
    prg, sites = mixed_variant_prg(ref, 60, 6, max_alleles=12)
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_haplotype_reads(ref, sites, 600, 40, 80, 7)]
    seeds = master_seeds(7, [len(reads)])
    want = expect_from(prg, 6, describe_tasks(prg, 6, reads, seeds), 1)
    ix = Index(prg, 6)
    roomy = run(ix, reads, seeds, 1)
    check(roomy, want, "roomy log")
    tiny = run(ix, reads, seeds, 1, chunk=150, log_cap_words=64)
    assert tiny[3].queue_counts()["log_replays"] > 0
    check(tiny, want, "tiny log")
    assert tiny[0] == roomy[0] and tiny[0]["grouped"] == roomy[0]["grouped"] == want["cov"]["grouped"]


# ---- 5. the limit off ------------------------------------------------------------------------------------------------
def test_a_limit_taken_back_leaves_an_untouched_engines_result():
    _, _, reads, seeds = case("nested_ladder")
    ix = index_of("nested_ladder")
    cov, out = limit_off("nested_ladder")
    assert not (out & 0xC0).any()
    qm = Quasimapper(ix)
    qm.record_outcomes(True)
    assert qm.max_candidates == 0
    qm.set_max_candidates(3)
    assert qm.max_candidates == 3
    qm.set_max_candidates(0)
    run_feed(qm, reads, seeds, "bytes")
    assert canonical_cov(qm.coverage()) == cov and qm.outcomes().tolist() == out.tolist()
    # only while nothing is recorded
    assert qm.lib.gmx_engine_set_max_candidates(qm.h, 2) == GMX_EINVAL and b"gmx_engine_reset" in qm.lib.gmx_last_error()
    with pytest.raises(GmxError):
        qm.set_max_candidates(2)
    assert qm.max_candidates == 0
    qm.reset()
    qm.set_max_candidates(2)  # the reset keeps the limit it is given now
    run_feed(qm, reads, seeds, "bytes")
    assert without_stats(canonical_cov(qm.coverage())) == expectation("nested_ladder", 2)["cov"]
    assert qm.outcomes().tolist() == expectation("nested_ladder", 2)["bytes"].tolist()
    qm.reset()
    assert qm.max_candidates == 2


# ---- 6. engine groups ------------------------------------------------------------------------------------------------
def test_a_group_sets_all_its_members_and_sums_to_the_single_engine():
    _, _, reads, seeds = case("ladder")
    ix = index_of("ladder")
    single = run(ix, reads, seeds, 2)
    for devices in ([0, 0], [0, 0, 0]):
        grp = QuasimapperGroup(ix, devices)
        grp.record_outcomes(True)
        grp.set_max_candidates(2)
        members = [C.c_void_p(grp.lib.gmx_group_engine(grp.h, i)) for i in range(len(devices))]
        assert [grp.lib.gmx_engine_max_candidates(m) for m in members] == [2] * len(devices)
        cuts = [0, 101, 250, len(reads)]
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            flat, offs = flatten_reads(reads[lo:hi])
            if j == 1:
                pk = pack_reads(flat, offs, pinned=True)
                grp.map_reads_packed(pk, seeds[lo:hi])
            else:
                grp.map_reads(flat, offs, seeds[lo:hi])
        grp.allreduce()
        assert canonical_cov(grp.coverage()) == single[0], devices
        assert grp.outcomes().tolist() == single[1].tolist() == expectation("ladder", 2)["bytes"].tolist()
        # its members have recorded: none is changed
        assert grp.lib.gmx_group_set_max_candidates(grp.h, 5) == GMX_EINVAL
        assert [grp.lib.gmx_engine_max_candidates(m) for m in members] == [2] * len(devices)
        # all or none: the first member is reset and would take the value, the second refuses, the first goes back
        assert grp.lib.gmx_engine_reset(members[0]) == 0
        assert grp.lib.gmx_group_set_max_candidates(grp.h, 5) == GMX_EINVAL
        assert [grp.lib.gmx_engine_max_candidates(m) for m in members] == [2] * len(devices)
        pk.close()
        grp.close()


# ---- 7. gram genotype --max_candidates -------------------------------------------------------------------------------
COV_FILES = ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")


def parsed_coverage(out):
    """The three coverage files in the form of common.canonical_*'s allele_sum, allele_base and grouped."""
    d = out / "coverage"
    asum = [[int(x) for x in line.split()] for line in (d / COV_FILES[0]).read_text().splitlines()]
    pb = json.loads((d / COV_FILES[1]).read_text())["allele_base_counts"]
    gp = json.loads((d / COV_FILES[2]).read_text())["grouped_allele_counts"]
    groups = {gid: tuple(ids) for gid, ids in gp["allele_groups"].items()}
    return dict(allele_sum=asum, allele_base=pb, grouped=[{groups[g]: c for g, c in site.items()} for site in gp["site_counts"]])


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from ingest_formats_common import gram
    from test_ingest import bgzf
    d = tmp_path_factory.mktemp("max_candidates_cli")
    prg, k, reads, _ = case("ladder")
    (d / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    fq = "".join(f"@r{i}\n{''.join('ACGT'[b - 1] for b in r)}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()
    (d / "s.fq").write_bytes(fq)
    (d / "s.bgzf.fq.gz").write_bytes(bgzf(fq, block=9000))

    def run_gram(name, reads_file="s.fq", seed="1", extra=(), env=None, ok=True):
        out = d / name
        r = gram("genotype", "--gram_dir", str(d), "--reads", str(d / reads_file), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", str(k),
                 "--genotype_dir", str(out), "--seed", seed, *extra, env=env or {})
        assert (r.returncode == 0) == ok, (name, r.stdout)
        return out, r
    return run_gram


def files(out):
    return [(out / "coverage" / f).read_bytes() for f in COV_FILES]


def test_gram_max_candidates_one_does_not_depend_on_the_seed(cli):
    a, _ = cli("limit1-seed1", seed="1", extra=["--max_candidates", "1"])
    b, _ = cli("limit1-seed2", seed="2", extra=["--max_candidates", "1"])
    assert files(a) == files(b)
    off1, _ = cli("off-seed1", seed="1")
    off2, _ = cli("off-seed2", seed="2")
    assert files(off1) != files(off2)
    want = expectation("ladder", 1)
    got = parsed_coverage(a)
    for key in got:
        assert got[key] == want["cov"][key], key
    js = json.loads((a / "read_filter.json").read_text())
    codes = np.concatenate([want["bytes"] & 3, (want["bytes"] >> 2) & 3])
    assert js == {"max_candidates": 1, "reads": 400, "tasks_mapped": int((codes == 3).sum()), "tasks_left_out": 128}
    assert not (a / "read_outcomes.bin").exists() and not (a / "read_outcomes.json").exists()
    # without the flag: no filter file, and the coverage of the engine with the limit off under gram's seeds
    assert not (off1 / "read_filter.json").exists() and not (off1 / "read_outcomes.bin").exists()
    prg, k, reads, _ = case("ladder")
    off = expect_from(prg, k, describe_tasks(prg, k, reads, master_seeds(1, [len(reads)])), 0)
    got = parsed_coverage(off1)
    for key in got:
        assert got[key] == off["cov"][key], key


CLI_ROUTES = [("two-engines", "s.fq", ["--devices", "0,0"], {"GMX_TEXT_CHUNK": "6000"}),
              ("recordings", "s.fq", ["--read_outcomes", "--read_positions"], {}),
              ("strands", "s.fq", ["--strand_coverage", "--strand_bias"], {}),
              ("bgzf", "s.bgzf.fq.gz", [], {})]


@pytest.mark.parametrize("name,reads_file,extra,env", CLI_ROUTES, ids=[r[0] for r in CLI_ROUTES])
def test_gram_max_candidates_on_other_routes(cli, name, reads_file, extra, env):
    from test_read_outcomes import parse_outcomes_file
    from test_read_positions import parse_positions_file
    ref, _ = cli("limit1-seed1", seed="1", extra=["--max_candidates", "1"])
    out, _ = cli(name, reads_file, "1", ["--max_candidates", "1", *extra], env)
    assert files(out) == files(ref)
    assert json.loads((out / "read_filter.json").read_text()) == json.loads((ref / "read_filter.json").read_text())
    if name == "recordings":
        want = expectation("ladder", 1)
        assert parse_outcomes_file((out / "read_outcomes.bin").read_bytes()).tolist() == want["bytes"].tolist()
        pos = parse_positions_file((out / "read_positions.bin").read_bytes()).astype(np.uint32)
        left = np.zeros(pos.shape, dtype=bool)  # a left-out task's record does not depend on the seed; gram's seeds are not the case's
        for t in want["left_out"]:
            left[t >> 1, 2 * (t & 1):2 * (t & 1) + 2] = True
        assert (pos[left] == want["positions"][left]).all() and (pos[:, [1, 3]] == want["positions"][:, [1, 3]]).all()
    else:
        assert not (out / "read_outcomes.bin").exists()


@pytest.mark.parametrize("value", ["0", "x"])
def test_gram_refuses_a_bad_limit(cli, value):
    out, r = cli("bad-" + value, extra=["--max_candidates", value], ok=False)
    assert r.returncode == 1 and "max_candidates" in r.stdout and not (out / "coverage" / COV_FILES[0]).exists()

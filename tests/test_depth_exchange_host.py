"""Depth past 16 bits through the host side of the exchange (no GPU): the deep case of depth_common.py through the host
emulation, through gramtools_amd.distributed under gloo with 2 and 3 ranks (shard, all-reduce of the raw uint32 totals, all-gather
of the logs, finalise ON THE TOTAL), and through the dumps. No rank's share of the deep allele reaches 65 536, the total does:
a rank that finalised its own share (wrapped, saturated) before the sum, or a sum narrower than the totals, cannot pass.
test_depth_exchange.py is the device side of the same case."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from common import canonical_cov, flatten_reads, hostemu_map
from depth_common import (DEEP_ALLELE, FOUR_LIMBS, K, MASTER_SEED, N_READS, VALUE_SETS, VARIANTS, deep_of, deep_prg, deep_reads, deep_seeds,
                          oracle_shard, python_recombine, split_limbs)
from gramtools_amd import Index
from gramtools_amd.distributed import allreduce_raw, quasimap_reads_sharded, shard_range
from gramtools_amd.quasimap import (allele_base_json, dump_allele_base, dump_allele_sum, dump_grouped_allele_counts, grouped_json,
                                    hash_allele_groups)


@pytest.fixture(autouse=True)
def _log_for_six_alleles(monkeypatch):
    monkeypatch.setenv("GMX_DENSE_MAX_ALLELES", "5")  # the six-allele site on the append log, the two-allele site dense


@pytest.fixture(scope="module")
def cases():
    """Per variant: the reads and the oracle of the whole job (one run each), plus the oracle of every rank's shard."""
    prg, seeds = deep_prg(), deep_seeds()
    out = {}
    for v in VARIANTS:
        reads = deep_reads(v)
        shards = {w: [oracle_shard(prg, reads, seeds, *shard_range(N_READS, w, r)) for r in range(w)] for w in (2, 3)}
        out[v] = dict(reads=reads, want=oracle_shard(prg, reads, seeds), shards=shards)
    return dict(prg=prg, seeds=seeds, by_variant=out)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dumps(cov):
    return dict(allele_sum=dump_allele_sum(cov), allele_base=dump_allele_base(cov), grouped=dump_grouped_allele_counts(cov))


def _worker(rank, world, port, prg, jobs, poked, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), GMX_DENSE_MAX_ALLELES="5")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        reads_of = lambda f, o: [f[int(o[i]):int(o[i + 1])] for i in range(len(o) - 1)]
        ix = Index(prg, K, threads=1)
        assert ix.uses_grouped_log
        for name, flat, offs in jobs:
            mine = {}

            def map_shard(r, o, seeds):
                raw, _, rc = hostemu_map(prg, K, reads_of(r, o), seeds, return_raw=True)
                assert rc == 0
                mine["deep"] = int(raw["allele_sum"][DEEP_ALLELE[name]])  # this rank's own share, before the exchange
                return raw
            cov = quasimap_reads_sharded(ix, flat, offs, MASTER_SEED, map_shard, dist=dist)
            q.put((name, rank, dict(canon=canonical_cov(cov), dumps=_dumps(cov), own_deep=mine["deep"],
                                    raw_deep=int(cov.raw_allele_sum[DEEP_ALLELE[name]]))))
        if poked is not None:  # allreduce_raw alone, on counters no mapping job of a test reaches
            raw = dict(allele_sum=np.asarray(poked["allele_sum"][rank], dtype=np.uint32), per_base=np.zeros(1, np.uint32),
                       grouped=np.zeros(1, np.uint32), grouped_log=np.zeros(0, np.uint32),
                       stats=np.asarray(poked["stats"][rank], dtype=np.uint64))
            red = allreduce_raw(raw, dist)
            q.put(("poked", rank, dict(stats=[int(x) for x in red["stats"]], allele_sum=[int(x) for x in red["allele_sum"]],
                                       dtypes=(str(red["stats"].dtype), str(red["allele_sum"].dtype)))))
    finally:
        dist.destroy_process_group()


# counters from 2^32 on, a different counter carrying out of bit 32 / bit 48 on each rank; totals below 2^63 (the sum travels as int64)
POKED_STATS = [[2 ** 32 - 1, 1, 2 ** 48 - 1, 0xFFFF, 2 ** 33 + 5],
               [1, 2 ** 32 - 1, 1, 2 ** 32, 2 ** 47],
               [2 ** 40, 2 ** 32, 2 ** 48, 1, 3]]
POKED_ALLELE_SUM = [[40000, 0xFFFFFFFF, 65535], [40000, 1, 1], [7, 0, 65535]]  # uint32 totals: the sum wraps mod 2^32 like the device's


def _run_world(world, prg, jobs, poked=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, prg, jobs, poked, q)) for r in range(world)]
    for p in procs:
        p.start()
    n_msgs = world * (len(jobs) + (1 if poked is not None else 0))
    res = {}
    for _ in range(n_msgs):
        name, rank, val = q.get(timeout=180)
        res[(name, rank)] = val
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


@pytest.fixture(scope="module")
def gloo_runs(cases):
    """One spawn per world size maps both variants (and reduces the poked counters): {world: {(name, rank): result}}."""
    jobs = [(v, *flatten_reads(cases["by_variant"][v]["reads"])) for v in VARIANTS]
    with pytest.MonkeyPatch.context() as mpatch:
        mpatch.setenv("GMX_DENSE_MAX_ALLELES", "5")
        return {w: _run_world(w, cases["prg"], jobs, dict(stats=POKED_STATS[:w], allele_sum=POKED_ALLELE_SUM[:w])) for w in (2, 3)}


def _total_deep(case, variant):
    """Condition (a) from the oracle alone: its uint16 counters are exact on the halves (asserted below 65 536), whose sum is the
    job's raw total."""
    halves = [deep_of(s, variant) for s in case["shards"][2]]
    assert all(h < 65536 for h in halves)
    return sum(halves)


@pytest.mark.parametrize("variant", VARIANTS)
def test_host_emulation_equals_the_oracle_past_16_bits(cases, variant):
    case = cases["by_variant"][variant]
    want = case["want"]
    total = _total_deep(case, variant)
    print(f"{variant}: deep total {total}, oracle shows {deep_of(want, variant)}")
    assert total > 65535                                                              # (a)
    assert deep_of(want, variant) == total - 65536                                    # the oracle wrapped it
    assert all(c == 65535 for c in want["allele_base"][0][DEEP_ALLELE[variant]])      # ... and saturated its bases
    assert want["grouped"][0][(DEEP_ALLELE[variant],)] == total - 65536
    got, _, rc = hostemu_map(cases["prg"], K, case["reads"], cases["seeds"])
    assert rc == 0 and got == want
    raw, _, rc = hostemu_map(cases["prg"], K, case["reads"], cases["seeds"], return_raw=True)
    assert rc == 0 and int(raw["allele_sum"][DEEP_ALLELE[variant]]) == total          # uint32 on the accumulating side
    assert raw["grouped_log"].size > 0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("world", [2, 3])
def test_ranks_under_gloo_finalise_the_total_not_their_shares(cases, gloo_runs, world, variant):
    case = cases["by_variant"][variant]
    want = case["want"]
    total = _total_deep(case, variant)
    shares = [deep_of(s, variant) for s in case["shards"][world]]
    print(f"{variant}, {world} ranks: shares {shares}, total {total}")
    assert total > 65535 and all(s < 65536 for s in shares) and sum(shares) == total  # (a), (b)
    for rank in range(world):
        got = gloo_runs[world][(variant, rank)]
        assert got["own_deep"] == shares[rank]
        assert got["raw_deep"] == total
        assert got["canon"] == want, rank


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("world", [2, 3])
def test_dumps_of_the_reduced_totals_equal_the_oracles(cases, gloo_runs, world, variant):
    want = cases["by_variant"][variant]["want"]
    deep = DEEP_ALLELE[variant]
    asum = "".join(" ".join(str(c) for c in site) + "\n" for site in want["allele_sum"])
    abase = allele_base_json(want["allele_base"]) + "\n"
    grouped = grouped_json(want["grouped"], hash_allele_groups(want["grouped"])) + "\n"
    assert int(asum.split()[deep]) == _total_deep(cases["by_variant"][variant], variant) - 65536  # wrapped in the text
    assert "65535" in abase                                                                        # saturated in the text
    for rank in range(world):
        got = gloo_runs[world][(variant, rank)]["dumps"]
        assert got["allele_sum"] == asum and got["allele_base"] == abase and got["grouped"] == grouped, rank


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_raw_adds_counters_from_2_to_the_32_on(gloo_runs, world):
    """The read counters are uint64 and a whole-genome job's pass 2^32; the coverage totals are uint32 and wrap as the device's."""
    want_stats = [sum(POKED_STATS[r][c] for r in range(world)) for c in range(5)]
    want_asum = [sum(POKED_ALLELE_SUM[r][c] for r in range(world)) % 2 ** 32 for c in range(3)]
    assert max(want_stats) < 2 ** 63 and min(want_stats) >= 2 ** 32
    assert any(sum(POKED_STATS[r][c] % 2 ** 32 for r in range(world)) >= 2 ** 32 for c in range(5))  # a carry out of bit 32
    for rank in range(world):
        got = gloo_runs[world][("poked", rank)]
        assert got["stats"] == want_stats and got["allele_sum"] == want_asum
        assert got["dtypes"] == ("uint64", "uint32")


def _genotype_worker(variant, q):
    os.environ["GMX_DENSE_MAX_ALLELES"] = "5"
    from gramtools_amd import Coverage, QuasimapReadsStats
    from gramtools_amd.quasimap import Genotyped
    prg = deep_prg()
    raw, _, rc = hostemu_map(prg, K, deep_reads(variant), deep_seeds(), return_raw=True)
    cov = Coverage(Index(prg, K, threads=1), raw["allele_sum"], raw["per_base"], raw["grouped"], raw["grouped_log"],
                   QuasimapReadsStats(*(int(x) for x in raw["stats"])))
    g = Genotyped(cov, 0.0001, "haploid")
    q.put((rc, cov.depth_stats(), [g.site(i) for i in range(2)]))


@pytest.mark.parametrize("variant", VARIANTS)
def test_genotyping_the_deep_coverage_returns(cases, variant):
    """The stage's simulated confidences (add_percentiles: a PRG of fewer than 10 000 sites) draw coverage from a negative
    binomial of the job's depth: mean 41 165 here, so that many a draw lies above 65 535. Drawn as uint16, as the reference
    draws them, such a draw is rejected for ever and `gram genotype` never returned on a job this deep. In a child process, so
    that a relapse fails instead of hanging the suite."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_genotype_worker, args=(variant, q))
    p.start()
    p.join(timeout=120)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("genotyping a site deeper than 65 535 reads did not return")
    assert p.exitcode == 0
    rc, depth, sites = q.get(timeout=10)
    assert rc == 0 and depth["mean"] > 40000 and depth["variance"] > depth["mean"]  # (the negative-binomial branch)
    assert sites[0]["HAPG"] == [[DEEP_ALLELE[variant]]] and sites[1]["HAPG"] == [[0]]  # the deep allele is called
    grouped = cases["by_variant"][variant]["want"]["grouped"][0]  # the stage sees the oracle's wrapped counts
    assert sites[0]["COV"][0][-1] == grouped[(DEEP_ALLELE[variant],)] < 65536 and sites[0]["DP"] == [sum(grouped.values())]
    assert all(0. <= s["GT_CONF_PERCENTILE"][0] <= 100. for s in sites)

def test_value_sets_can_tell_a_wrong_recombination():
    """depth_common.VALUE_SETS (poked into the device counters by test_depth_exchange.py) hold what the issue lists, and at least one (set, R) separates `+` from `|` in the recombination and an
    unmasked limb sum from one masked to 16 bits (most values do NOT: 0xFFFF * 2 | next limb << 16 is often the same number)."""
    flat = [v for vals, _ in VALUE_SETS for v in vals]
    for must in (0, 1, 0xFFFF, 0x10000, 2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1, FOUR_LIMBS):
        assert must in flat
    assert len(set(split_limbs(FOUR_LIMBS))) == 4 and 0 not in split_limbs(FOUR_LIMBS)
    tells_or = tells_mask = 0
    for vals, ranks in VALUE_SETS:
        for r in ranks:
            for v in vals:
                assert r * v < 2 ** 64
                words = [l * r for l in split_limbs(v)]
                assert max(words) < 2 ** 32 and python_recombine(words, int.__add__) == r * v
                tells_or += python_recombine(words, int.__or__) != r * v
                tells_mask += python_recombine([w & 0xFFFF for w in words], int.__add__) != r * v
    assert tells_or >= 3 and tells_mask >= 10, (tells_or, tells_mask)

"""Depth past 16 bits through everything on the device side that ADDS totals (test_depth_limits.py pins the uint16 semantics on
one engine and one dense site only): the read counters' 16-bit limbs (gmx_coverage_reduce_begin / _end, gmx_stats_limbs_kernel)
against Python integers up to 2^64, the peer-copy exchange of a group (gmx_add_u32_kernel, the log's counted records), the two
strands' blocks, a log drained thousands of times, the world-size-1 exchanges and `gram genotype --devices`. The case is
depth_common.py's: no member's, rank's or strand's share of the deep allele reaches 65 536, the total does, so a step that
finalised a share, dropped a carry or narrowed a sum cannot pass. test_depth_exchange_host.py is the host side."""
import json
import os
import socket

import numpy as np
import pytest

from common import canonical_cov, flatten_reads
from depth_common import (DEEP_ALLELE, K, MASTER_SEED, N_READS, STAT_KEYS, VARIANTS, carrying_counters, deep_of, deep_prg, deep_reads,
                          deep_seeds, oracle_shard, oracle_strand_deep, split_limbs, VALUE_SETS)
from gramtools_amd import Index, Quasimapper, QuasimapperGroup, pack_reads
from gramtools_amd.distributed import shard_range
from gramtools_amd.quasimap import LOG_COUNTED, LOG_PAD, LOG_REVERSE

pytestmark = pytest.mark.gpu

FIRST_CALL = 40000  # the reads go over in two calls of different sizes: 40 000 as bytes, 65 536 as bit planes


@pytest.fixture(autouse=True)
def _log_for_six_alleles(monkeypatch):
    monkeypatch.setenv("GMX_DENSE_MAX_ALLELES", "5")  # the six-allele site on the append log, the two-allele site dense


def deep_index(prg):
    ix = Index(prg, K)
    assert ix.uses_grouped_log and int(ix.n_alleles[0]) == 6 and int(ix.grouped_off[1]) != 0xFFFFFFFF
    return ix


def member_read_sets(n_members):
    """The read indices every member of a group gets from the two calls (contiguous ranges of each call, gmx_multi.hip)."""
    sets = [[] for _ in range(n_members)]
    for lo, hi in ((0, FIRST_CALL), (FIRST_CALL, N_READS)):
        for m in range(n_members):
            a, b = shard_range(hi - lo, n_members, m)
            sets[m] += list(range(lo + a, lo + b))
    return sets


@pytest.fixture(scope="module")
def cases():
    """Per variant: reads, the oracle of the whole job (one run), the oracle of every member's reads for groups of 2 and 3 (their
    uint16 counts of the deep allele are exact: asserted below 65 536), the per-strand counts of the deep allele."""
    prg, seeds = deep_prg(), deep_seeds()
    out = {}
    for v in VARIANTS:
        reads = deep_reads(v)
        shares = {}
        for n in (2, 3):
            shares[n] = []
            for idx in member_read_sets(n):
                canon = oracle_shard(prg, [reads[i] for i in idx], seeds[idx])
                shares[n].append(dict(deep=deep_of(canon, v), stats=canon["stats"]))
        out[v] = dict(reads=reads, want=oracle_shard(prg, reads, seeds), shares=shares, strands=oracle_strand_deep(prg, reads, seeds, v))
    return dict(prg=prg, seeds=seeds, by_variant=out)


def feed_two_calls(target, reads, seeds):
    """40 000 reads through map_reads, the other 65 536 through map_reads_packed (page-locked bit planes)."""
    flat, offs = flatten_reads(reads)
    cut = int(offs[FIRST_CALL])
    target.map_reads(flat[:cut], offs[:FIRST_CALL + 1], seeds[:FIRST_CALL])
    pk = pack_reads(flat[cut:], offs[FIRST_CALL:] - offs[FIRST_CALL], pinned=True)
    target.map_reads_packed(pk, seeds[FIRST_CALL:])
    return pk


def raws(cov):
    return [np.asarray(x).astype(np.uint64) for x in (cov.raw_allele_sum, cov.raw_per_base, cov.raw_grouped)]


def log_records(log):
    """{(site, ids, reverse): count} of a grouped log; every record must be a counted one and every key appear once."""
    out, i = {}, 0
    log = [int(x) for x in log]
    while i < len(log):
        if log[i] == LOG_PAD:
            i += 1
            continue
        site, w = log[i], log[i + 1]
        assert w & LOG_COUNTED, "a record worth +1 in a fetched log"
        n = w & ~(LOG_COUNTED | LOG_REVERSE)
        key = (site, tuple(log[i + 4:i + 4 + n]), bool(w & LOG_REVERSE))
        assert key not in out
        out[key] = log[i + 2] | (log[i + 3] << 32)
        i += 4 + n
    return out


@pytest.fixture(scope="module")
def single(cases):
    """One engine with per-strand recording and the default (roomy) log on the whole job, per variant: the strands' raw arrays and
    logs, the totals. One run each, shared: a single engine needs seconds for this job (every read appends to the log, and
    CoverLogPart::log_reserve is one compare-and-swap loop on one cursor for all of them)."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GMX_DENSE_MAX_ALLELES", "5")
        ix = deep_index(cases["prg"])
        for v in VARIANTS:
            qm = Quasimapper(ix)
            qm.record_strands(True)
            pk = feed_two_calls(qm, cases["by_variant"][v]["reads"], cases["seeds"])
            qm.sync()
            out[v] = dict(strand_raw=[raws(qm.coverage(strand=s)) for s in (0, 1)], strand_log=[log_records(qm.grouped_log(s)) for s in (0, 1)],
                          total_raw=raws(qm.coverage()), total=canonical_cov(qm.coverage()), total_log=log_records(qm.grouped_log()),
                          log_replays=qm.queue_counts()["log_replays"])
            pk.close()
            qm.close()
    return out


# ---- 1. the counters' limbs against Python integers ------------------------------------------------------------------
def _set_counters(s, vals):
    import torch
    s.copy_(torch.from_numpy(np.asarray(vals, dtype=np.uint64).view(np.int64).copy()))
    torch.cuda.synchronize()


def _get_counters(s):
    import torch
    torch.cuda.synchronize()
    return [int(x) for x in s.cpu().numpy().view(np.uint64)]


@pytest.mark.parametrize("strands", [False, True], ids=["one-block", "two-blocks"])
def test_counter_limbs_against_python_integers(cases, strands):
    import torch
    from gramtools_amd.distributed import fused_coverage_tensor, stats_tensor
    ix = deep_index(cases["prg"])
    qm = Quasimapper(ix)
    if strands:
        qm.record_strands(True)
    reads = cases["by_variant"]["one-base"]["reads"][:600]  # (accumulator words that are not all zero)
    flat, offs = flatten_reads(reads)
    qm.map_reads(flat, offs, cases["seeds"][:600])
    qm.sync()
    t, s = fused_coverage_tensor(qm), stats_tensor(qm)
    n_acc = t.numel() - 32
    assert s.numel() == 5 and s.data_ptr() == t.data_ptr() + 4 * t.numel()
    assert _get_counters(s) == [1200, 0, 600, 0, 600]
    acc = t[:n_acc].cpu()
    assert int(acc.ne(0).sum()) > 0 and (not strands or int(acc[n_acc // 2:].ne(0).sum()) > 0)
    for vals, ranks in VALUE_SETS:
        for r in ranks:
            _set_counters(s, vals)
            qm.reduce_begin()
            torch.cuda.synchronize()
            words = t[n_acc:].cpu().numpy().view(np.uint32)
            assert [int(x) for x in words[:20]] == [l for v in vals for l in split_limbs(v)], (vals, r)
            assert not words[20:].any()
            assert torch.equal(t[:n_acc].cpu(), acc)
            assert _get_counters(s) == list(vals)  # (the counters themselves stay while their limbs travel)
            summed = (words.astype(np.uint64) * np.uint64(r)).astype(np.uint32)  # what an all-reduce over r equal ranks leaves
            assert [int(x) for x in summed] == [int(x) * r for x in words]          # ... exactly: no limb sum passes 2^32
            t[n_acc:].copy_(torch.from_numpy(summed.view(np.int32).copy()))
            torch.cuda.synchronize()
            qm.reduce_end()
            assert _get_counters(s) == [r * v for v in vals], (vals, r)
            assert torch.equal(t[:n_acc].cpu(), acc)
            st = qm.coverage().stats  # ... and through the library's own read-out
            assert [st.all_reads_count, st.skipped_reads_count, st.missing_kmer_reads_count, st.no_extension_reads_count,
                    st.exact_mapped_reads_count] == [r * v for v in vals]
    qm.reset()
    assert _get_counters(stats_tensor(qm)) == [0] * 5
    assert qm.coverage().stats.as_dict() == dict.fromkeys(STAT_KEYS, 0)
    qm.close()


# ---- 2. a group adds poked counters ----------------------------------------------------------------------------------
@pytest.mark.parametrize("strands", [False, True], ids=["one-block", "two-blocks"])
@pytest.mark.parametrize("devices,values", [([0, 0], (2 ** 32 - 1, 1)), ([0, 0, 0], (2 ** 48 - 1, 2 ** 48 - 1, 2))], ids=["2-engines", "3-engines"])
def test_a_group_adds_poked_counters(cases, devices, values, strands):
    """Counter c of member m holds values[(m + c) % n]: the large values, hence the limbs that carry, sit in another member for
    every counter. The sums are 2^32 and 2^49."""
    from gramtools_amd.distributed import stats_tensor
    n = len(devices)
    grp = QuasimapperGroup(deep_index(cases["prg"]), devices)
    assert grp.lib.gmx_group_uses_rccl(grp.h) == 0  # engines of one device: peer copies and gmx_add_u32_kernel
    if strands:
        grp.record_strands(True)
    poked = [[values[(m + c) % n] for c in range(5)] for m in range(n)]
    for m in range(n):
        view = grp._member(m)
        try:
            view.sync()
            _set_counters(stats_tensor(view), poked[m])
        finally:
            view.h = None  # the group owns the engine
    for m in range(n):
        assert list(grp.coverage(m).stats.as_dict().values()) == poked[m]
    grp.allreduce()
    want = [sum(poked[m][c] for m in range(n)) for c in range(5)]
    assert want == [sum(values)] * 5 and sum(values) in (2 ** 32, 2 ** 49)
    for m in range(n):
        cov = grp.coverage(m)
        assert list(cov.stats.as_dict().values()) == want, m
        assert not any(x.any() for x in raws(cov))  # nothing was mapped: the blocks stay zero
    grp.close()


# ---- 3. a group at real depth against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("strands", [False, True], ids=["strands-off", "strands-on"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["2-engines", "3-engines"])
def test_a_group_at_real_depth_equals_the_oracle(cases, single, devices, variant, strands):
    case = cases["by_variant"][variant]
    want, n, deep = case["want"], len(devices), DEEP_ALLELE[variant]
    grp = QuasimapperGroup(deep_index(cases["prg"]), devices)
    assert grp.lib.gmx_group_uses_rccl(grp.h) == 0
    if strands:
        grp.record_strands(True)
    pk = feed_two_calls(grp, case["reads"], cases["seeds"])
    before = [grp.coverage(m) for m in range(n)]
    # (b) from oracle runs of the members' reads, (c) from the members' own counters; the members' raws agree with both
    shares = [sh["deep"] for sh in case["shares"][n]]
    total = sum(shares)
    member_stats = [c.stats.as_dict() for c in before]
    carrying = carrying_counters(member_stats)
    upper = [k for k in STAT_KEYS if max(ms[k] for ms in member_stats) >= 1 << 16]
    low_sums = {k: sum(ms[k] & 0xFFFF for ms in member_stats) for k in STAT_KEYS}
    print(f"{variant}, {n} members, strands {strands}: deep shares {shares}, total {total}; counters {member_stats}; "
          f"low-limb sums {low_sums}; carrying with a non-zero upper limb {carrying}")
    assert total > 65535 and all(s < 65536 for s in shares)                                  # (a), (b)
    assert [int(c.raw_allele_sum[deep]) for c in before] == shares
    assert member_stats == [sh["stats"] for sh in case["shares"][n]]
    # (c): some member's counter has a non-zero upper limb and some counter's lowest limbs carry when added. With two members
    # one counter (`all`: 40 000 + 40 000) does both. Three members of this job cannot have that: their `all` is a third of
    # 211 072 each (lowest limbs 4 822 + 4 822 + 4 820), their `exact_mapped` carries (35 179 + 35 179 + 35 178) from below 2^16.
    assert upper and max(low_sums.values()) >= 1 << 16
    if n == 2:
        assert carrying
    grp.allreduce()
    sums = [sum(x) for x in zip(*(raws(c) for c in before))]
    for m in range(n):
        cov = grp.coverage(m)
        assert canonical_cov(cov) == want, m
        assert all((got == s).all() for got, s in zip(raws(cov), sums)), m
        assert int(cov.raw_allele_sum[deep]) == total > 65535
        exported = log_records(grp.export_grouped_log(m))
        both = [exported.get((0, (deep,), rev), 0) for rev in (False, True)]
        assert sum(both) == total and (strands or both[1] == 0), (m, both)
        if strands:
            assert both == [single[variant]["strand_log"][s][(0, (deep,), False)] for s in (0, 1)]
    assert all((a == b).all() for a, b in zip(sums, single[variant]["total_raw"]))
    if strands:
        fwd_rev = case["strands"]
        print(f"{variant}: deep allele per strand {fwd_rev}")
        assert sum(fwd_rev) == total and all(x < 65536 for x in fwd_rev)                     # (b) per strand, from the oracle
        for m in range(n):
            per_strand = [raws(grp.coverage(m, strand=s)) for s in (0, 1)]
            for s in (0, 1):
                assert all((a == b).all() for a, b in zip(per_strand[s], single[variant]["strand_raw"][s])), (m, s)
                assert log_records(grp.grouped_log(m, strand=s)) == single[variant]["strand_log"][s], (m, s)
                assert int(per_strand[s][0][deep]) == fwd_rev[s] < 65536
                assert log_records(grp.grouped_log(m, strand=s))[(0, (deep,), False)] == fwd_rev[s]
            assert all(((a + b) == t).all() for a, b, t in zip(per_strand[0], per_strand[1], sums)), m
    pk.close()
    grp.close()


# ---- 4. one engine, a log drained thousands of times -----------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_engine_with_a_tiny_and_a_roomy_log(cases, single, variant):
    """A log of 64 words is drained and its batch replayed thousands of times; the roomy log (the default, the `single` fixture's
    run) never. Both hold the oracle's counts, and one counted record of more than 65 535."""
    case, deep = cases["by_variant"][variant], DEEP_ALLELE[variant]
    flat, offs = flatten_reads(case["reads"])
    qm = Quasimapper(deep_index(cases["prg"]), log_cap_words=64, max_batch_reads=20000)
    qm.map_reads(flat, offs, cases["seeds"])
    cov = qm.coverage()
    assert canonical_cov(cov) == case["want"] == single[variant]["total"]
    assert qm.queue_counts()["log_replays"] > 0 and single[variant]["log_replays"] == 0
    rec = log_records(cov.raw_grouped_log)
    assert rec == single[variant]["total_log"]
    assert rec[(0, (deep,), False)] == int(cov.raw_allele_sum[deep]) > 65535
    qm.close()


# ---- 5. world size 1 -------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world_size_1_exchanges_leave_the_deep_job_unchanged(cases, monkeypatch, strands=True):
    """gmx_comm_* with one rank, then the torch route with a one-rank stand-in: counters -> limbs -> counters with non-zero
    upper limbs, the log exported and merged; nothing may change. With per-strand recording: the limbs sit behind the second
    block and the log travels in its exchange form."""
    import torch
    import torch.distributed as dist
    from gramtools_amd.distributed import CoverageComm, allreduce_device_coverage

    class OneRank:  # a process group of one: the all-reduce is the identity
        def all_reduce(self, t):
            pass

        def get_world_size(self):
            return 1

    torch.cuda.init()
    case = cases["by_variant"]["one-base"]
    qm = Quasimapper(deep_index(cases["prg"]))
    if strands:
        qm.record_strands(True)
    pk = feed_two_calls(qm, case["reads"], cases["seeds"])
    qm.sync()
    before = qm.coverage()
    assert canonical_cov(before) == case["want"]
    assert before.stats.all_reads_count >= 1 << 16 and before.stats.exact_mapped_reads_count >= 1 << 16
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        comm = CoverageComm(qm, dist)
        comm.allreduce()
        qm.sync()
        comm.close()
    finally:
        dist.destroy_process_group()
    for step in ("gmx_comm", "torch"):
        if step == "torch":
            allreduce_device_coverage(qm, OneRank())
            qm.sync()
        after = qm.coverage()
        assert after.stats.as_dict() == before.stats.as_dict() == case["want"]["stats"], step
        assert all((a == b).all() for a, b in zip(raws(after), raws(before))), step
        assert log_records(after.raw_grouped_log) == log_records(before.raw_grouped_log), step
        assert canonical_cov(after) == case["want"], step
    pk.close()
    qm.close()


# ---- 6. gram genotype ------------------------------------------------------------------------------------------------
def _allele_sum_rows(text):
    return [[int(x) for x in line.split()] for line in text.splitlines()]


def test_gram_one_device_and_two_engines_write_the_same_deep_files(cases, tmp_path, variant="one-base"):
    """Fresh child processes: `--device 0` against `--devices 0,0`, both with --strand_coverage. The reference's three files
    hold the oracle's numbers (wrapped, saturated, wrapped); the strand files are raw and add up to the unwrapped total."""
    from ingest_formats_common import gram
    case = cases["by_variant"][variant]
    want, deep = case["want"], DEEP_ALLELE[variant]
    (tmp_path / "prg").write_bytes(np.asarray(cases["prg"], dtype="<u4").tobytes())
    with open(tmp_path / "r.fq", "w") as fh:
        fh.write("".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate("".join("ACGT"[b - 1] for b in r) for r in case["reads"])))
    runs = []
    for name, dev in (("one", ["--device", "0"]), ("two", ["--devices", "0,0"])):
        out = tmp_path / name
        r = gram("genotype", "--gram_dir", str(tmp_path), "--reads", str(tmp_path / "r.fq"), "--sample_id", "s", "--ploidy", "haploid",
                 "--kmer_size", str(K), "--genotype_dir", str(out), "--seed", str(MASTER_SEED), "--max_threads", "4", "--strand_coverage", *dev)
        assert r.returncode == 0, r.stdout
        files = {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}
        runs.append(dict(counts=[l for l in r.stdout.splitlines() if l.startswith("Count ")],
                         files={rel: b for rel, b in files.items() if rel.startswith(("coverage", "genotype")) or rel.endswith("read_stats.json")}))
    one, two = runs
    assert one["counts"] == two["counts"] and [int(l.split()[-1]) for l in two["counts"]] == [want["stats"][k] for k in STAT_KEYS]
    assert sorted(one["files"]) == sorted(two["files"])
    cov_files = ["allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json", "allele_sum_coverage.forward",
                 "allele_sum_coverage.reverse", "allele_base_coverage.forward.json", "allele_base_coverage.reverse.json"]
    assert all(os.path.join("coverage", f) in two["files"] for f in cov_files) and "read_stats.json" in two["files"]
    assert any(rel.startswith("genotype") for rel in two["files"])
    for rel in two["files"]:
        assert one["files"][rel] == two["files"][rel], rel
    got = {f: two["files"][os.path.join("coverage", f)].decode() for f in cov_files}
    assert _allele_sum_rows(got["allele_sum_coverage"]) == want["allele_sum"]                               # wrapped
    assert json.loads(got["allele_base_coverage.json"])["allele_base_counts"] == want["allele_base"]       # saturated
    grouped = json.loads(got["grouped_allele_counts_coverage.json"])["grouped_allele_counts"]
    groups = {g: tuple(ids) for g, ids in grouped["allele_groups"].items()}
    assert [{groups[g]: c for g, c in site.items()} for site in grouped["site_counts"]] == want["grouped"]  # wrapped
    fwd, rev = (_allele_sum_rows(got[f"allele_sum_coverage.{s}"]) for s in ("forward", "reverse"))
    total = sum(sh["deep"] for sh in case["shares"][2])
    assert (fwd[0][deep], rev[0][deep]) == case["strands"] and fwd[0][deep] + rev[0][deep] == total > 65535
    assert want["allele_sum"][0][deep] == total - 65536
    bf, br = (json.loads(got[f"allele_base_coverage.{s}.json"])["allele_base_counts"] for s in ("forward", "reverse"))
    assert [a + b for a, b in zip(bf[0][deep], br[0][deep])] == [total] * len(bf[0][deep])

"""Coverage per strand (gmx_engine_record_strands, include/gmx.h): two accumulator blocks — what the reads as given added and
what their reverse complements added — chosen by the task's parity at every place a coverage kernel sets its accumulator.

The oracle for one strand is the oracle itself: Oracle.quasimap_read maps ONE orientation, so the forward block is
quasimap_read(read_i, seed_i) over all reads and the reverse block quasimap_read(reverse_complement(read_i), seed_i) (the
reference uses a read's seed for both orientations, quasimap.cpp:159-194). Clean reads only: quasimap_read does not skip."""
import ctypes as C
import json

import numpy as np
import pytest

from common import canonical_cov, flatten_reads, oracle_map
from oracle import Oracle
from gramtools_amd import GmxError, Index, Quasimapper, QuasimapperGroup, _lib, master_seeds, pack_reads
from gramtools_amd.quasimap import GROUPED_LOG
from gramtools_amd.synth import (bracket_to_ints, mixed_variant_prg, nested_prg, random_ref, simulate_graph_reads,
                                 simulate_haplotype_reads, simulate_snp_reads, snp_prg)
from test_many_instances import tandem_prg, tandem_reads

pytestmark = pytest.mark.gpu

GMX_EINVAL = -1


def revcomp(r):
    return (5 - np.asarray(r, dtype=np.uint8))[::-1].copy()


def oracle_view(o, log_sites=()):
    """What a strand's Coverage holds, from an oracle: no read counters, no depth; the grouped counts of the sites on the
    grouped log are not split (gmx.h), so they are left out on both sides."""
    grouped = o.grouped()
    for s in log_sites:
        grouped[s] = {}
    return dict(allele_sum=o.allele_sum(), grouped=grouped, per_base={n["first_pos"]: n["cov"] for n in o.per_base_nodes()},
                allele_base=o.allele_base_non_nested())


def cov_view(cov):
    return dict(allele_sum=cov.allele_sum_coverage, grouped=cov.grouped_allele_counts, per_base=cov.per_base_by_first_pos(),
                allele_base=cov.allele_base_coverage)


def log_sites_of(ix):
    return [s for s in range(ix.n_sites) if int(ix.grouped_off[s]) == GROUPED_LOG]


_oracle_cache = {}


def oracle_strands(key, prg, k, reads, seeds, ix):
    """(forward view, reverse view) of the per-orientation oracle passes, computed once per case."""
    if key not in _oracle_cache:
        views = []
        for strand in (0, 1):
            o = Oracle(prg, k)
            for r, s in zip(reads, seeds):
                o.quasimap_read(revcomp(r) if strand else np.asarray(r, dtype=np.uint8), int(s))
            views.append(oracle_view(o, log_sites_of(ix)))
            o.close()
        _oracle_cache[key] = tuple(views)
    return _oracle_cache[key]


def run(ix, reads, seeds, strands=True, chunk=0, **kw):
    qm = Quasimapper(ix, **kw)
    if strands:
        qm.record_strands(True)
    feed(qm, reads, seeds, chunk)
    return qm


def feed(qm, reads, seeds, chunk=0):
    step = chunk or max(len(reads), 1)
    for lo in range(0, len(reads), step):
        flat, offs = flatten_reads(reads[lo:lo + step])
        qm.map_reads(flat, offs, np.ascontiguousarray(seeds[lo:lo + step], dtype=np.uint32))
    qm.sync()


def raw(cov):
    return [np.asarray(x).copy() for x in (cov.raw_allele_sum, cov.raw_per_base, cov.raw_grouped)]


def same_raw(a, b):
    return all((x == y).all() for x, y in zip(raw(a), raw(b)))


def check_split(key, prg, k, reads, seeds, ix=None, **kw):
    """Both blocks against the per-orientation oracle, the total against the whole oracle and an engine with recording off."""
    ix = ix or Index(prg, k)
    want_f, want_r = oracle_strands(key, prg, k, reads, seeds, ix)
    qm = run(ix, reads, seeds, **kw)
    fwd, rev, total = qm.coverage(strand=0), qm.coverage(strand=1), qm.coverage()
    assert cov_view(fwd) == want_f, "forward block"
    assert cov_view(rev) == want_r, "reverse block"
    assert fwd.raw_grouped_log.size == 0 and rev.raw_grouped_log.size == 0
    assert int(fwd.raw_allele_sum.sum()) > 0 and int(rev.raw_allele_sum.sum()) > 0  # (a block written to the wrong strand cannot hide)
    off = run(ix, reads, seeds, strands=False, **kw)
    plain = off.coverage()
    assert same_raw(total, plain) and (total.raw_grouped_log == plain.raw_grouped_log).all()
    assert total.stats.as_dict() == plain.stats.as_dict() == fwd.stats.as_dict()  # the read counters are not split
    for a, b, t in zip(raw(fwd), raw(rev), raw(total)):
        assert ((a + b) == t).all()
    return qm, total


# ---- 1. the split against the oracle ---------------------------------------------------------------------------------
def flat_case():
    """The issue's flat PRG (2 kb, 20 SNP sites, a third multi-allelic) with one site of 9 alleles appended — its grouped counts
    go to the log, gmx_cover_jump_kernel declines reads over it (gmx_cover_single_rest_kernel) — and 300 reads of 60 bases."""
    prg, *_ = snp_prg(random_ref(2000, 4), 20, 5, multi_allelic_frac=0.3)
    ints = [int(x) for x in prg]
    m = max(ints) + 1 + (max(ints) % 2)  # next odd marker
    rng = np.random.default_rng(12)
    site = [m]
    for a in range(9):
        site += [1 + a // 4 % 4, 1 + a % 4, 1 + (a * 3 + 1) % 4] + [m + 1]
    ints += [int(x) for x in rng.integers(1, 5, 40)] + site + [int(x) for x in rng.integers(1, 5, 80)]
    prg = np.asarray(ints, dtype=np.uint32)
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_graph_reads(prg, 300, 60, 7, rc_prob=0.5)]
    return prg, 6, reads


def nested_case():
    prg = bracket_to_ints(nested_prg(71, n_top=12, max_depth=3))
    return prg, 5, [np.asarray(r, dtype=np.uint8) for r in simulate_graph_reads(prg, 200, 20, 3)]


def test_flat_prg_both_blocks_against_the_per_orientation_oracle():
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    assert ix.uses_grouped_log and len(log_sites_of(ix)) == 1
    seeds = (np.arange(len(reads), dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)
    qm, total = check_split("flat", prg, k, reads, seeds, ix=ix)
    counts = qm.queue_counts()
    # the compact records (gmx_cover_jump_kernel, and gmx_cover_single_rest_kernel for what it declines: the reads over the
    # 9-allele site, whose records are in the log)
    assert counts["mapped"] - counts["cover_general"] > 100, counts
    assert total.raw_grouped_log.size > 0
    assert canonical_cov(total) == oracle_map(prg, k, reads, seeds)


def test_nested_prg_both_blocks_against_the_per_orientation_oracle():
    prg, k, reads = nested_case()
    seeds = (np.arange(len(reads), dtype=np.uint64) * 40503 + 17).astype(np.uint32)
    qm, total = check_split("nested", prg, k, reads, seeds)
    counts = qm.queue_counts()
    # compact records (gmx_cover_single_kernel<true>) and what it hands on: gmx_cover_one_kernel, then the general instances
    assert counts["mapped"] - counts["cover_general"] > 0 and counts["cover_general"] > 0, counts
    assert canonical_cov(total) == oracle_map(prg, k, reads, seeds)


# ---- 2. draws and tiers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_copies", [10, 40, 300, 6000], ids=["cooperative", "cooperative-rejects", "large-capacity-tier", "last-tier"])
def test_reads_with_many_mapping_instances_split_as_the_oracle_splits_them(n_copies):
    """Tandem copies of a unit with a SNP site: a read has one mapping instance per copy and the seeded draw picks one. 10
    copies: the cooperative kernel (up to 16 units per task); 40: its rejects, the serial instance; 300: the large-capacity
    pass and the largest scratch; 6 000: the heap-backed last tier. tandem_reads mixes strands."""
    prg, unit, site_at, alt = tandem_prg(n_copies, 60, 5)
    reads = tandem_reads(unit, site_at, alt, 100, 6)
    seeds = master_seeds(11, [len(reads)])
    qm, _ = check_split(("tandem", n_copies), prg, 8, reads, seeds)
    counts = qm.queue_counts()
    if n_copies == 10:  # what the large-capacity search mapped: 10 units per task, within the cooperative kernel's 16
        assert counts["big_mapped"] >= 4 and counts["cover_overflow"] == 0 and counts["huge_search"] + counts["huge_cover"] == 0, counts
    elif n_copies == 40:  # more than 16 units: rejected to the serial instance, whose regular scratch they exceed as well
        assert counts["big_mapped"] >= 4 and counts["cover_overflow"] >= 4 and counts["huge_search"] + counts["huge_cover"] == 0, counts
    elif n_copies == 300:
        assert counts["big_mapped"] + counts["cover_overflow"] > 0 and counts["huge_search"] + counts["huge_cover"] == 0
    else:
        assert counts["huge_search"] + counts["huge_cover"] >= 4


def test_a_palindromic_read_adds_the_same_to_both_blocks():
    """A read that is its own reverse complement: both tasks are the same search with the same seed."""
    rng = np.random.default_rng(5)
    u, w = rng.integers(1, 5, 9, dtype=np.uint8), rng.integers(1, 5, 8, dtype=np.uint8)
    left, right = rng.integers(1, 5, 30, dtype=np.uint8), rng.integers(1, 5, 30, dtype=np.uint8)
    tail = np.concatenate([w, revcomp(w), [4], revcomp(u)])
    prg = np.asarray([*left, *u, 5, 1, 6, 2, 6, *tail, *right], dtype=np.uint32)  # the site: A | C
    read = np.concatenate([u, [1], tail]).astype(np.uint8)
    assert (revcomp(read) == read).all()
    qm = run(Index(prg, 6), [read], np.asarray([77], dtype=np.uint32))
    fwd, rev = qm.coverage(strand=0), qm.coverage(strand=1)
    assert same_raw(fwd, rev)
    assert fwd.allele_sum_coverage == [[1, 0]] and int(fwd.raw_per_base.sum()) == 1
    assert qm.coverage().allele_sum_coverage == [[2, 0]]


# ---- 3. the redo paths: log replay, the twin workspace ---------------------------------------------------------------
def log_case():
    ref = random_ref(3000, 5)
    prg, sites = mixed_variant_prg(ref, 60, 6, max_alleles=12)
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_haplotype_reads(ref, sites, 600, 40, 80, 7)]
    return prg, 6, reads


def test_a_replayed_task_records_into_its_own_strand(monkeypatch):
    """Sites on the grouped log, a log of 64 words and batches of 150 reads: tasks that find the log full are redone whole
    after a drain, from their queue entries — which carry the task id, hence the strand."""
    prg, k, reads = log_case()
    ix = Index(prg, k)
    assert ix.uses_grouped_log
    seeds = master_seeds(5, [len(reads)])
    monkeypatch.setenv("GMX_TWIN", "0")
    roomy = run(ix, reads, seeds)
    assert roomy.queue_counts()["log_replays"] == 0
    want = [roomy.coverage(strand=0), roomy.coverage(strand=1), roomy.coverage()]
    want_f, want_r = oracle_strands("log", prg, k, reads, seeds, ix)
    assert cov_view(want[0]) == want_f and cov_view(want[1]) == want_r
    monkeypatch.setenv("GMX_TWIN", "1")
    tiny = run(ix, reads, seeds, chunk=300, log_cap_words=64, max_batch_reads=150)
    assert tiny.queue_counts()["log_replays"] > 0
    got = [tiny.coverage(strand=0), tiny.coverage(strand=1), tiny.coverage()]
    for g, w in zip(got, want):
        assert same_raw(g, w)
    assert got[2].grouped_allele_counts == want[2].grouped_allele_counts


def test_the_twin_workspace_records_into_the_engines_two_blocks(monkeypatch):
    """GMX_TWIN=1, launches of 64 reads taken by the two workspaces in turn: the twin's alias of the block and its offset
    follow record_strands, also when it is switched after the twin was made."""
    prg, k, reads = nested_case()
    ix = Index(prg, k)
    seeds = (np.arange(len(reads), dtype=np.uint64) * 40503 + 17).astype(np.uint32)
    want_f, want_r = oracle_strands("nested", prg, k, reads, seeds, ix)
    monkeypatch.setenv("GMX_TWIN", "0")
    one = run(ix, reads, seeds)
    assert not one.lib.gmx_engine_second_stream(one.h)
    monkeypatch.setenv("GMX_TWIN", "1")
    two = run(ix, reads, seeds, chunk=64)
    assert two.lib.gmx_engine_second_stream(two.h)
    for strand, want in ((0, want_f), (1, want_r)):
        assert cov_view(two.coverage(strand=strand)) == want
        assert same_raw(two.coverage(strand=strand), one.coverage(strand=strand))
    assert same_raw(two.coverage(), one.coverage())


# ---- 4. forward-only engines -----------------------------------------------------------------------------------------
def test_forward_only_leaves_the_reverse_block_zero():
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    qm = run(ix, reads, seeds, forward_only=True)
    fwd, rev, total = qm.coverage(strand=0), qm.coverage(strand=1), qm.coverage()
    assert all(int(x.sum()) == 0 for x in raw(rev))
    assert same_raw(fwd, total) and int(fwd.raw_allele_sum.sum()) > 0
    assert same_raw(total, run(ix, reads, seeds, strands=False, forward_only=True).coverage())


# ---- 5. state rules --------------------------------------------------------------------------------------------------
def test_state_rules_resets_and_switching():
    import torch
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    lib = _lib.load()
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    buf = np.zeros(max(ix.info.n_allele_slots, 1), dtype=np.uint32)
    qm = Quasimapper(ix)
    assert lib.gmx_coverage_fetch_strand(qm.h, 0, u32(buf), None, None) == GMX_EINVAL  # recording is off
    assert lib.gmx_engine_record_strands(None, 1) == GMX_EINVAL and lib.gmx_coverage_fetch_strand(None, 0, None, None, None) == GMX_EINVAL
    feed(qm, reads, seeds)
    plain = qm.coverage()
    assert lib.gmx_engine_record_strands(qm.h, 1) == GMX_EINVAL  # reads were mapped
    assert b"reset" in lib.gmx_last_error()
    assert same_raw(qm.coverage(), plain)  # ... and nothing was lost
    qm.reset()
    qm.record_strands(True)
    assert lib.gmx_coverage_fetch_strand(qm.h, 2, u32(buf), None, None) == GMX_EINVAL
    feed(qm, reads, seeds)
    want = [qm.coverage(strand=0), qm.coverage(strand=1)]
    assert same_raw(qm.coverage(), plain) and int(want[1].raw_allele_sum.sum()) > 0
    with pytest.raises(GmxError):
        qm.record_strands(False)  # recorded: not now
    stream = torch.cuda.current_stream().cuda_stream

    def both_zero():
        return all(int(x.sum()) == 0 for s in (0, 1) for x in raw(qm.coverage(strand=s))) and qm.coverage().stats.as_dict()["all"] == 0

    qm.reset()
    assert both_zero()
    feed(qm, reads[:100], seeds[:100])
    qm.reset(stream=stream)  # queued; a reader issues it first
    assert both_zero()
    feed(qm, reads[:100], seeds[:100])
    qm.reset(stream=stream)  # queued, folded into the next batch's first kernel (launched on the same stream)
    flat, offs = flatten_reads(reads)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (flat, offs, seeds)]
    qm.map_reads_device(dev[0], dev[1].view(torch.int64), dev[2].view(torch.int32), len(reads), stream=stream)
    qm.sync()
    for s in (0, 1):
        assert same_raw(qm.coverage(strand=s), want[s]), "after the folded reset"
    # off / on / off / on, one engine: the same answers each time
    for on in (False, True, False, True):
        qm.reset(stream=stream) if on else qm.reset()
        qm.record_strands(on)
        feed(qm, reads, seeds)
        assert same_raw(qm.coverage(), plain), on
        if on:
            for s in (0, 1):
                assert same_raw(qm.coverage(strand=s), want[s])
        else:
            assert lib.gmx_coverage_fetch_strand(qm.h, 0, u32(buf), None, None) == GMX_EINVAL


# ---- 6. groups -------------------------------------------------------------------------------------------------------
def test_a_group_exchanges_both_blocks():
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    single = run(ix, reads, seeds)
    want = [single.coverage(strand=0), single.coverage(strand=1), single.coverage()]
    flat, offs = flatten_reads(reads)
    for devices in ([0, 0], [0, 0, 0]):
        grp = QuasimapperGroup(ix, devices)
        grp.record_strands(True)
        grp.map_reads(flat[:int(offs[120])], offs[:121], seeds[:120])
        pk = pack_reads(flat[int(offs[120]):], offs[120:] - offs[120], pinned=True)
        grp.map_reads_packed(pk, seeds[120:])
        grp.allreduce()
        for member in range(len(devices)):
            for s in (0, 1):
                assert same_raw(grp.coverage(member, strand=s), want[s]), (devices, member, s)
            total = grp.coverage(member)
            assert same_raw(total, want[2]) and total.stats.as_dict() == want[2].stats.as_dict()
            assert total.grouped_allele_counts == want[2].grouped_allele_counts
        pk.close()
        grp.close()


def test_a_group_whose_members_disagree_is_refused():
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    grp = QuasimapperGroup(ix, [0, 0])
    lib = grp.lib
    assert lib.gmx_group_record_strands(None, 1) == GMX_EINVAL
    assert lib.gmx_engine_record_strands(C.c_void_p(lib.gmx_group_engine(grp.h, 1)), 1) == 0  # one member only
    flat, offs = flatten_reads(reads)
    grp.map_reads(flat, offs, master_seeds(3, [len(reads)]))
    assert lib.gmx_group_allreduce(grp.h) == GMX_EINVAL and b"disagree" in lib.gmx_last_error()
    assert lib.gmx_group_record_strands(grp.h, 1) == GMX_EINVAL  # its members have recorded
    grp.close()


# ---- 7. gram genotype --strand_coverage ------------------------------------------------------------------------------
def parse_allele_sum(text):
    return [[int(x) for x in line.split()] for line in text.splitlines()]


@pytest.fixture(scope="module")
def cli_sample(tmp_path_factory):
    from ingest_formats_common import gram
    from test_ingest import bgzf
    d = tmp_path_factory.mktemp("strand_cli")
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    (d / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    reads = simulate_snp_reads(ref, pos, alts, n_alts, 6100, 60, 6)
    txt = ["".join("ACGT"[b - 1] for b in r) for r in reads]
    fq = "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(txt)).encode()
    (d / "s.fq").write_bytes(fq)
    (d / "s.bgzf.fq.gz").write_bytes(bgzf(fq, block=9000))

    def run_gram(name, reads_file, extra=()):
        out = d / name
        r = gram("genotype", "--gram_dir", str(d), "--reads", str(d / reads_file), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", "6",
                 "--genotype_dir", str(out), "--seed", "1234", *extra)
        assert r.returncode == 0, (name, r.stdout)
        return out

    ix = Index(prg, 6)
    qm = run(ix, list(reads), master_seeds(1234, [len(reads)]))
    return dict(run=run_gram, fwd=qm.coverage(strand=0), rev=qm.coverage(strand=1))


def files_of(out):
    """Every file of a run but the strand files, and the timing-free ones only (relative path -> bytes)."""
    found = {}
    for p in sorted(out.rglob("*")):
        rel = str(p.relative_to(out))
        if p.is_file() and ".forward" not in rel and ".reverse" not in rel:
            found[rel] = p.read_bytes()
    return found


@pytest.mark.parametrize("name,reads_file,extra", [("plain", "s.fq", []), ("bgzf", "s.bgzf.fq.gz", []), ("two-engines", "s.fq", ["--devices", "0,0"])])
def test_gram_strand_coverage_files(cli_sample, name, reads_file, extra):
    out = cli_sample["run"](name, reads_file, ["--strand_coverage", *extra])
    base = cli_sample["run"](name + "-noflag", reads_file, extra)
    cov = out / "coverage"
    fwd, rev = parse_allele_sum((cov / "allele_sum_coverage.forward").read_text()), parse_allele_sum((cov / "allele_sum_coverage.reverse").read_text())
    total = parse_allele_sum((cov / "allele_sum_coverage").read_text())
    assert len(fwd) == len(rev) == len(total) == 40
    assert [[(a + b) % 65536 for a, b in zip(f, r)] for f, r in zip(fwd, rev)] == total
    bf, br = (json.loads((cov / f"allele_base_coverage.{s}.json").read_text())["allele_base_counts"] for s in ("forward", "reverse"))
    bt = json.loads((cov / "allele_base_coverage.json").read_text())["allele_base_counts"]
    assert [[[min(a + b, 65535) for a, b in zip(x, y)] for x, y in zip(sf, sr)] for sf, sr in zip(bf, br)] == bt
    # raw totals: the engine's own blocks for these reads and seeds
    assert fwd == [[int(x) for x in site] for site in _raw_allele_sum(cli_sample["fwd"])]
    assert rev == [[int(x) for x in site] for site in _raw_allele_sum(cli_sample["rev"])]
    assert bf == cli_sample["fwd"].allele_base_coverage and br == cli_sample["rev"].allele_base_coverage  # (far below saturation)
    assert sum(map(sum, fwd)) > 0 and sum(map(sum, rev)) > 0
    # every pre-existing output is byte-identical to the run without the flag
    with_flag, without = files_of(out), files_of(base)
    assert sorted(with_flag) == sorted(without) and len(without) >= 6
    for rel in without:
        if rel.endswith("read_stats.json") or rel.startswith("coverage") or rel.startswith("genotype"):
            assert with_flag[rel] == without[rel], rel
    assert not (base / "coverage" / "allele_sum_coverage.forward").exists()


def _raw_allele_sum(cov):
    ix = cov.index
    return [cov.raw_allele_sum[o:o + n] for o, n in zip(ix.allele_sum_off, ix.n_alleles)]


def test_gram_strand_coverage_across_a_samples_list(cli_sample, tmp_path):
    """Two samples in one call: the engines stay in the mode, the reset between samples zeroes both blocks."""
    from ingest_formats_common import gram
    d = cli_sample["run"]("plain-again", "s.fq", ["--strand_coverage"]).parent
    lst = tmp_path / "samples.tsv"
    lst.write_text(f"a\t{tmp_path / 'a'}\t{d / 's.fq'}\nb\t{tmp_path / 'b'}\t{d / 's.bgzf.fq.gz'}\n")
    r = gram("genotype", "--gram_dir", str(d), "--samples_list", str(lst), "--ploidy", "diploid", "--kmer_size", "6", "--seed", "1234",
             "--strand_coverage")
    assert r.returncode == 0, r.stdout
    for s in ("a", "b"):
        for f in ("allele_sum_coverage.forward", "allele_sum_coverage.reverse", "allele_base_coverage.forward.json", "allele_base_coverage.reverse.json"):
            assert (tmp_path / s / "coverage" / f).read_bytes() == (d / "plain-again" / "coverage" / f).read_bytes(), (s, f)


# ---- 8. allocation failure -------------------------------------------------------------------------------------------
def test_strand_calls_survive_every_failed_allocation():
    """gmx_debug_fail_alloc makes the library's n-th HOST allocation throw. The switch has one on an engine whose last change of
    its allocation list was an allocation (a fresh engine; one that has just mapped): the list's growth, ahead of the device
    allocation. So every n gets a fresh engine. NOT covered: a failing hipMalloc (the "old block intact" branch behind that
    host allocation) — this hook cannot inject it."""
    from test_alloc_failure import GMX_ENOMEM, _count_allocs
    lib = _lib.load()
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    clean = run(ix, reads, seeds)
    want = [clean.coverage(strand=0), clean.coverage(strand=1)]
    plain = run(ix, reads, seeds, strands=False).coverage()
    probe = Quasimapper(ix)
    n = _count_allocs(lib, lambda: lib.gmx_engine_record_strands(probe.h, 1))
    assert n >= 1
    for nth in range(1, n + 1):
        qm = Quasimapper(ix)
        lib.gmx_debug_fail_alloc(nth)
        rc = lib.gmx_engine_record_strands(qm.h, 1)
        lib.gmx_debug_fail_alloc(0)
        assert rc == GMX_ENOMEM and lib.gmx_last_error(), (nth, rc)
        # the mode and the block are as they were: recording is off, the engine maps and reads back as one that never switched
        assert lib.gmx_coverage_fetch_strand(qm.h, 0, None, None, None) == GMX_EINVAL
        feed(qm, reads, seeds)
        got = qm.coverage()
        assert same_raw(got, plain) and got.stats.as_dict() == plain.stats.as_dict()
        qm.reset()
        qm.record_strands(True)  # ... and can still be switched
        feed(qm, reads, seeds)
        for s_ in (0, 1):
            assert same_raw(qm.coverage(strand=s_), want[s_])
    qm = clean

    def fetch():
        try:
            qm.coverage(strand=1)
            return 0
        except GmxError as e:
            return e.code
    n = _count_allocs(lib, fetch)
    assert n >= 1
    for nth in range(1, n + 1):
        lib.gmx_debug_fail_alloc(nth)
        rc = fetch()
        lib.gmx_debug_fail_alloc(0)
        assert rc == GMX_ENOMEM, (nth, rc)
    for s_ in (0, 1):
        assert same_raw(qm.coverage(strand=s_), want[s_])


def test_the_torch_exchange_refuses_a_tensor_of_the_replaced_block():
    from gramtools_amd.distributed import allreduce_device_coverage, fused_coverage_tensor

    class OneRank:  # a process group of one: the all-reduce is the identity
        def all_reduce(self, t):
            pass

        def get_world_size(self):
            return 1

    prg, k, reads = flat_case()
    qm = Quasimapper(Index(prg, k))
    stale = fused_coverage_tensor(qm)
    qm.record_strands(True)
    fresh = fused_coverage_tensor(qm)
    assert fresh.numel() == 2 * (stale.numel() - 32) + 32
    with pytest.raises(ValueError):
        allreduce_device_coverage(qm, OneRank(), tensor=stale)
    seeds = master_seeds(3, [len(reads)])
    feed(qm, reads, seeds)
    want = [qm.coverage(strand=0), qm.coverage(strand=1), qm.coverage()]
    allreduce_device_coverage(qm, OneRank(), tensor=fresh)  # counters -> limbs -> counters: nothing changes
    qm.sync()
    assert same_raw(qm.coverage(strand=0), want[0]) and same_raw(qm.coverage(strand=1), want[1])
    assert qm.coverage().stats.as_dict() == want[2].stats.as_dict()

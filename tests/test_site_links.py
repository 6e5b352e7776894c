"""Links between nearby sites (gmx_engine_record_links, include/gmx.h): for every read orientation that maps with
exactly one mapping instance, the allele pairs it shows at sites at most `span` site indices apart. The expectation comes from the
oracle alone (site_links_common.py). A task counts exactly once on every routine that finishes it — gmx_link_kernel over the compact
records, gmx_cover_task's single-instance shortcut, the one-lane kernel, the cooperative kernel, the tiers, the log replay, both
workspaces, every feed, engine groups and `gram genotype --site_links` — and the recording changes nothing else."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from common import canonical_cov, flatten_reads
from gramtools_amd import GmxError, Index, Quasimapper, QuasimapperGroup, link_matrix
from gramtools_amd.synth import bracket_to_ints
import site_links_common as slc
from test_read_outcomes import FEEDS, run_feed

pytestmark = pytest.mark.gpu

GMX_EINVAL = -1
u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


@functools.lru_cache(maxsize=None)
def index(wide=True):
    prg, k, _, _ = slc.case(wide)
    return Index(prg, k)


@functools.lru_cache(maxsize=None)
def checked_case():
    """The case, after the assertions on what it contains (before any GPU work)."""
    slc.check_case_contents()
    return slc.case()


def run(span, feed="bytes", chunk=0, strands=False, ambiguity=False, wide=True, order=None, **kw):
    """(link words or None, canonical coverage, engine); wide=False: the case without its 10-allele site (no log, two workspaces)"""
    checked_case()
    _, _, reads, seeds = slc.case(wide)
    if order is not None:  # the same reads with the same seeds, handed over in another order
        reads, seeds = [reads[i] for i in order], seeds[np.asarray(order)]
    qm = Quasimapper(index(wide), **kw)
    if strands:
        qm.record_strands(True)
    if ambiguity:
        qm.record_site_ambiguity(True)
    if span:
        qm.record_links(span)
    assert qm.link_span == span
    run_feed(qm, reads, seeds, feed, chunk)
    words = None
    if span:
        off, words = qm.links()
        assert off.tolist() == slc.expectation(span, wide)[0].tolist()
    return words, canonical_cov(qm.coverage()), qm


def same_block(got, want, note=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint32 and got.shape == want.shape, (note, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (note, [(int(w), int(got[w]), int(want[w])) for w in bad[:10]], int(got.sum()), int(want.sum()))


@functools.lru_cache(maxsize=None)
def plain():
    """An engine with recording off: coverage and the five counters."""
    return run(0)[1]


@functools.lru_cache(maxsize=None)
def span3():
    return run(3)[:2]


def test_single_instance_tasks_without_a_compact_record_reach_the_serial_instances():
    """With recording on, the one-lane kernel and the cooperative kernel leave a single-instance task that has a path to the serial
    instance of its queue, whose gmx_cover_task adds its pairs. The case must put such tasks there, or a missing hand-over would
    not show."""
    off, on = run(0)[2].queue_counts(), run(3)[2].queue_counts()
    print("recording off", off, "recording on", on)
    assert off["cover_general"] == on["cover_general"] > 0
    assert on["coop_rejected"] >= off["coop_rejected"] + 10  # (about 30 of the case's 171 general tasks have one instance and a path)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------
def test_the_block_is_the_oracles_word_for_word():
    words, cov = span3()
    same_block(words, slc.expectation(3)[1], "span 3")
    assert words.any() and cov == plain()
    n_alleles = index().n_alleles
    one, seven = run(1)[0], run(7)[0]
    same_block(one, slc.expectation(1)[1], "span 1")
    same_block(seven, slc.expectation(7)[1], "span 7")
    off1, off3, off7 = (slc.expectation(s)[0] for s in (1, 3, 7))
    some = 0
    for s in range(index().n_sites):
        for d in (1, 2, 3):
            m3 = link_matrix(n_alleles, off3, words, s, d)
            assert (link_matrix(n_alleles, off7, seven, s, d) == m3).all(), (s, d)
            if d == 1:
                assert (link_matrix(n_alleles, off1, one, s, 1) == m3).all(), s
            some += int(m3.sum())
    assert some == int(words.sum()) and int(seven.sum()) > some


# ---- 2. feeds, workspaces, a queued reset ----------------------------------------------------------------------------
@pytest.mark.parametrize("twin,wide", [("0", True), ("1", True), ("0", False), ("1", False)])
def test_every_feed_and_both_workspaces(monkeypatch, twin, wide):
    """(An index with a site that uses the grouped log has no second workspace: the case without its 10-allele site has one.)"""
    import torch
    monkeypatch.setenv("GMX_TWIN", twin)
    checked_case()
    _, _, reads, seeds = slc.case(wide)
    want = slc.expectation(3, wide)[1]
    off_cov = run(0, wide=wide)[1]
    assert want.any()
    for feed in FEEDS:
        for chunk in (0, 97):
            words, cov, qm = run(3, feed=feed, chunk=chunk, wide=wide)
            assert bool(qm.lib.gmx_engine_second_stream(qm.h)) == (twin == "1" and not wide)
            same_block(words, want, (feed, chunk, twin))
            assert cov == off_cov, (feed, chunk, twin)  # the totals and the five counters of an engine with recording off
            if chunk:  # a queued reset: the block starts again, the span stays
                qm.reset(stream=torch.cuda.current_stream().cuda_stream)
                run_feed(qm, reads, seeds, feed, chunk)
                assert qm.link_span == 3
                same_block(qm.links()[1], want, (feed, "after a queued reset", twin))
                assert canonical_cov(qm.coverage()) == off_cov


# ---- 3. routes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", ["GMX_NO_COVER_JUMP", "GMX_NO_COOP", "GMX_NO_COVER_ONE"])
def test_other_routes_give_the_same_block(monkeypatch, var):
    """The walk instead of the geometry records; the serial instances instead of the cooperative kernel; the general instances
    instead of the one-lane kernel."""
    monkeypatch.setenv(var, "1")
    fresh = Index(*slc.case()[:2])  # (GMX_NO_COVER_JUMP is read when the engine is created; the index is the same)
    qm = Quasimapper(fresh)
    qm.record_links(3)
    _, _, reads, seeds = checked_case()
    run_feed(qm, reads, seeds, "bytes")
    same_block(qm.links()[1], slc.expectation(3)[1], var)
    assert canonical_cov(qm.coverage()) == plain()


# ---- 4. tiers --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tier_case():
    """300 tandem copies of a 60-base unit, each with its own two-allele site (test_many_instances.tandem_prg). A read that begins
    in the left flank and ends inside the second or third copy has ONE mapping instance and two or three loci, but its backward
    search starts inside the array with 300 candidates: it leaves the fast pass for the larger tiers."""
    import itertools
    from test_many_instances import tandem_prg
    prg, unit, site_at, alt = tandem_prg(300, 60, 5)
    left = np.asarray(prg[10:40], dtype=np.uint8)
    reads = []
    for copies in (2, 3):
        for i, combo in enumerate(itertools.product((0, 1), repeat=copies)):
            body = []
            for c in combo:
                u = unit.copy()
                if c:
                    u[site_at] = alt
                body.append(u)
            r = np.concatenate([left] + body)[:left.size + 60 * (copies - 1) + site_at + 6].astype(np.uint8)
            reads.append((5 - r[::-1]).astype(np.uint8) if i % 2 else r)
    from gramtools_amd import master_seeds
    return prg, reads, master_seeds(7, [len(reads)])


def test_a_task_counts_once_whichever_tier_finishes_it():
    """(The main case cannot be made to leave the fast pass, whatever the pools: its paths fit the per-lane pools, whose sizes are
    fixed, and `max_states` / `max_path_nodes` size only the tiers behind them. Hence this input of its own: two-allele sites only.)
    Default pools against small ones, which send the same tasks on to the heap-backed last tier. A task turned away by one tier
    and finished by the next must have counted once, and never in both gmx_link_kernel and gmx_cover_task."""
    prg, reads, seeds = tier_case()
    ix = Index(prg, 8)
    tasks = slc.describe(prg, 8, reads)
    assert sum(1 for _, n, loci, _ in tasks if n == 1 and len(loci) == 2) >= 4 and sum(1 for _, n, loci, _ in tasks if n == 1 and len(loci) == 3) >= 8
    _, want = slc.block_of(ix.n_alleles, 3, slc.matrices_of(ix.n_alleles, tasks, 3))
    assert int(want.sum()) == 4 * 1 + 8 * 3

    def go(**kw):
        qm = Quasimapper(ix, **kw)
        qm.record_links(3)
        run_feed(qm, reads, seeds, "bytes")
        return qm.links()[1], canonical_cov(qm.coverage()), qm.queue_counts()
    big, small = go(), go(max_states=64, max_path_nodes=128)
    print("default pools", big[2], "small pools", small[2])
    assert big[2]["overflow_probe"] + big[2]["overflow_extend"] >= len(reads) and big[2]["huge_search"] + big[2]["huge_cover"] == 0
    assert small[2]["huge_search"] >= len(reads)
    same_block(big[0], want, "default pools against the oracle")
    same_block(small[0], want, "small pools against the oracle")
    assert small[1] == big[1]


# ---- 5. log replay ---------------------------------------------------------------------------------------------------
def test_a_tiny_grouped_log_replays_without_counting_twice():
    """The reads that cross the 10-allele site first: the first launch of 150 reads appends more than the log's 64 words."""
    roomy = span3()
    wide_site = int(np.flatnonzero(slc.oracle_alleles() > 8)[0])
    crosses = [any(s == wide_site for s, _ in slc.described()[2 * i][2] + slc.described()[2 * i + 1][2]) for i in range(len(slc.case()[2]))]
    assert 3 * sum(crosses) > 64 and sum(crosses) <= 150
    order = sorted(range(len(crosses)), key=lambda i: not crosses[i])
    tiny = run(3, chunk=150, log_cap_words=64, order=order)
    assert tiny[2].queue_counts()["log_replays"] > 0
    same_block(tiny[0], roomy[0], "tiny log against roomy log")
    assert tiny[1] == roomy[1]


# ---- 6. switching ----------------------------------------------------------------------------------------------------
def test_switching_only_while_nothing_is_recorded_and_the_span_survives_a_reset():
    _, _, reads, seeds = checked_case()
    ix = index()
    qm = Quasimapper(ix)
    lib = qm.lib
    n3 = int(slc.expectation(3)[0][-1])
    buf = np.zeros(n3 + 8, dtype=np.uint32)
    assert lib.gmx_engine_links(qm.h) == 0
    assert lib.gmx_coverage_fetch_links(qm.h, u32(buf), n3) == GMX_EINVAL and b"gmx_engine_record_links" in lib.gmx_last_error()  # off
    for span in (8, -1):
        assert lib.gmx_engine_record_links(qm.h, span) == GMX_EINVAL and b"span" in lib.gmx_last_error()
    with pytest.raises(GmxError):
        qm.record_links(8)
    qm.record_links(3)
    qm.record_links(0)
    qm.record_links(5)
    qm.record_links(3)
    assert lib.gmx_engine_links(qm.h) == 3
    assert lib.gmx_coverage_fetch_links(qm.h, u32(buf), n3 + 1) == GMX_EINVAL and b"n_words" in lib.gmx_last_error()
    assert not qm.links()[1].any()
    run_feed(qm, reads, seeds, "bytes")
    same_block(qm.links()[1], slc.expectation(3)[1], "first job")
    assert lib.gmx_engine_record_links(qm.h, 0) == GMX_EINVAL and b"gmx_engine_reset" in lib.gmx_last_error()
    assert lib.gmx_engine_record_links(qm.h, 4) == GMX_EINVAL
    assert lib.gmx_engine_links(qm.h) == 3
    same_block(qm.links()[1], slc.expectation(3)[1], "a refused switch leaves the counts")
    qm.reset()
    assert lib.gmx_engine_links(qm.h) == 3 and not qm.links()[1].any()  # a reset zeroes the block and keeps the span
    run_feed(qm, reads[:200], seeds[:200], "bytes")
    qm.reset()
    qm.record_links(1)  # allowed again after a reset
    run_feed(qm, reads, seeds, "bytes")
    same_block(qm.links()[1], slc.expectation(1)[1], "span 1 after a reset")
    qm.reset()
    qm.record_links(0)
    run_feed(qm, reads, seeds, "bytes")
    assert canonical_cov(qm.coverage()) == plain()


def test_a_nested_index_is_refused():
    ix = Index(bracket_to_ints("acgtacgtta[ac,t[g,c]a]ttgacca[a,g]ccatgca"), 4)
    qm = Quasimapper(ix)
    assert qm.lib.gmx_engine_record_links(qm.h, 3) == GMX_EINVAL and b"flat" in qm.lib.gmx_last_error()
    assert qm.link_span == 0


# ---- 7. with the other two switches of the block's layout ------------------------------------------------------------
def test_combined_with_strands_and_site_ambiguity():
    words, cov, qm = run(3, strands=True, ambiguity=True)
    same_block(words, span3()[0], "with record_strands and record_site_ambiguity")
    assert cov == plain()
    fwd, rev, total = qm.coverage(strand=0), qm.coverage(strand=1), qm.coverage()
    assert ((fwd.raw_allele_sum + rev.raw_allele_sum) == total.raw_allele_sum).all() and fwd.raw_allele_sum.any() and rev.raw_allele_sum.any()
    assert ((fwd.raw_per_base + rev.raw_per_base) == total.raw_per_base).all()
    assert ((fwd.raw_grouped + rev.raw_grouped) == total.raw_grouped).all()
    drawn, passed = qm.site_ambiguity()
    _, _, alone = run(0, ambiguity=True)
    d0, p0 = alone.site_ambiguity()
    assert drawn.tolist() == d0.tolist() and passed.tolist() == p0.tolist() and (drawn.any() or passed.any())


# ---- 8. engine groups ------------------------------------------------------------------------------------------------
def test_a_group_sums_to_the_single_engine():
    _, _, reads, seeds = checked_case()
    grp = QuasimapperGroup(index(), [0, 0])
    grp.record_links(3)
    members = [C.c_void_p(grp.lib.gmx_group_engine(grp.h, i)) for i in range(2)]
    assert [grp.lib.gmx_engine_links(m) for m in members] == [3, 3]
    cuts = [0, 101, 350, len(reads)]
    for lo, hi in zip(cuts, cuts[1:]):
        flat, offs = flatten_reads(reads[lo:hi])
        grp.map_reads(flat, offs, seeds[lo:hi])
    grp.allreduce()
    same_block(grp.links(0)[1], span3()[0], "member 0 after the exchange")
    assert canonical_cov(grp.coverage()) == plain()
    assert grp.lib.gmx_group_record_links(grp.h, 0) == GMX_EINVAL  # its members have recorded: none is changed
    assert [grp.lib.gmx_engine_links(m) for m in members] == [3, 3]
    grp.close()


def test_a_group_whose_members_differ_in_span_does_not_exchange():
    _, _, reads, seeds = checked_case()
    grp = QuasimapperGroup(index(), [0, 0])
    grp.record_links(3)
    member = C.c_void_p(grp.lib.gmx_group_engine(grp.h, 1))
    assert grp.lib.gmx_engine_record_links(member, 2) == 0  # one member's span changed behind the group's back
    flat, offs = flatten_reads(reads[:50])
    grp.map_reads(flat, offs, seeds[:50])
    assert grp.lib.gmx_group_allreduce(grp.h) == GMX_EINVAL and b"gmx_group_record_links" in grp.lib.gmx_last_error()
    grp.close()


# ---- 9. gram genotype --site_links -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    from ingest_formats_common import gram
    d = tmp_path_factory.mktemp("site_links_cli")
    prg, k, reads, _ = checked_case()
    (d / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    (d / "s.fq").write_text("".join(f"@r{i}\n{''.join('ACGT'[b - 1] for b in r)}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)))
    nested = d / "nested"
    nested.mkdir()
    (nested / "prg").write_bytes(np.array(bracket_to_ints("acgtacgtta[ac,t[g,c]a]ttgacca[a,g]ccatgca"), dtype="<u4").tobytes())

    def run_gram(name, extra=(), env=None, gram_dir=d, ok=True):
        out = d / name
        r = gram("genotype", "--gram_dir", str(gram_dir), "--reads", str(d / "s.fq"), "--sample_id", "s", "--ploidy", "diploid", "--kmer_size", str(k),
                 "--genotype_dir", str(out), "--seed", "1", *extra, env=env or {})
        assert (r.returncode == 0) == ok, (name, r.returncode, r.stdout)
        return out, r
    run_gram.dir = d
    return run_gram


def all_files(out):
    return {str(p.relative_to(out)): p.read_bytes() for p in out.rglob("*") if p.is_file()}


def test_gram_writes_the_links(cli):
    out, _ = cli("links3", extra=["--site_links", "3"])
    js = json.loads((out / "coverage" / "site_links.json").read_text())
    assert list(js) == ["span", "links"] and js["span"] == 3
    n_alleles = index().n_alleles
    off, words = slc.expectation(3)  # (one mapping instance: the counts depend on no seed)
    again = np.zeros_like(words)
    pairs = []
    for s, t, rows in js["links"]:
        m = np.asarray(rows, dtype=np.uint32)
        assert m.shape == link_matrix(n_alleles, off, words, s, t - s).shape and m.any(), (s, t)
        at = slc.matrix_start(slc.oracle_alleles(), off, s, t - s)
        again[at:at + m.size] = m.reshape(-1)
        pairs.append((s, t))
    same_block(again, words, "site_links.json re-expanded")
    same_block(again, span3()[0], "site_links.json against the engine's fetch")
    assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
    summary = json.loads((out / "site_links.json").read_text())
    assert summary == {"span": 3, "sites": int(index().n_sites), "linkable_sites": int((n_alleles <= 8).sum()), "pairs_with_count": len(pairs),
                       "count": int(words.sum())}
    # two engines write the same two files
    two, _ = cli("links3-two-engines", extra=["--site_links", "3", "--devices", "0,0"], env={"GMX_TEXT_CHUNK": "6000"})
    for f in ("coverage/site_links.json", "site_links.json"):
        assert (two / f).read_bytes() == (out / f).read_bytes(), f
    # without the flag: the other files, byte for byte, and no new one
    plain_out, _ = cli("no-links")
    with_flag, without = all_files(out), all_files(plain_out)
    assert sorted(with_flag) == sorted(list(without) + ["coverage/site_links.json", "site_links.json"])
    for f, data in without.items():
        assert with_flag[f] == data, f


def test_gram_refuses_a_nested_prg_with_the_engines_message(cli):
    out, r = cli("links-nested", extra=["--site_links", "3"], gram_dir=cli.dir / "nested", ok=False)
    assert r.returncode == 1 and "flat PRGs only" in r.stdout, r.stdout

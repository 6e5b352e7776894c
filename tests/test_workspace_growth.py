"""The batch workspace as one value and the slot ring of the host feeds (gmx_engine_state.h: GmxWorkspace, gmx_engine::grow,
GmxFeedSlot), seen from outside: what a grown engine computes, and what it owns (gmx_engine_debug_owned_bytes) after a growth
that did not come about.
"""
import numpy as np
import pytest

from common import oracle_map, canonical_cov
from gramtools_amd import _lib, Index, Quasimapper, master_seeds, pack_reads, pack_reads_2bit
from gramtools_amd.synth import flat_offsets, random_ref, simulate_snp_reads, snp_prg, mixed_variant_prg, simulate_haplotype_reads

pytestmark = pytest.mark.gpu

N, LEN = 3000, 150


@pytest.fixture(scope="module")
def snp_case():
    """A flat SNP PRG of 6000 bases (test_alloc_failure._small_prg), 3000 reads of 150 bases, and what the byte feed makes of
    them on a fresh engine — the reference of this module, computed once."""
    ref = random_ref(6000, 11)
    prg, pos, alts, n_alts = snp_prg(ref, 60, 5)
    reads = np.ascontiguousarray(simulate_snp_reads(ref, pos, alts, n_alts, N, LEN, 5))
    seeds = master_seeds(7, [N])
    ix = Index(prg, 6)
    fresh = Quasimapper(ix)
    fresh.map_reads(reads.reshape(-1), flat_offsets(N, LEN), seeds)
    return ix, reads, seeds, canonical_cov(fresh.coverage())


def _map_first(qm, reads, seeds, n):
    qm.map_reads(reads[:n].reshape(-1), flat_offsets(n, LEN), seeds[:n])  # (one launch; the call returns synchronised)


def test_a_workspace_that_grew_computes_what_a_fresh_one_does(snp_case):
    """500, 1000, 2000 reads, a reset, 3000 reads: the workspace, the staging buffers and the bit planes grow on the way, and
    the last call's coverage is that of an engine that was given it alone."""
    ix, reads, seeds, want = snp_case
    for steps in ((500, 1000, 2000), (500,)):  # (1000 reads fit the first workspace, 2000 and 3000 each swap a fresh one in)
        qm = Quasimapper(ix)
        for n in steps:
            _map_first(qm, reads, seeds, n)
        qm.reset()
        _map_first(qm, reads, seeds, N)
        assert canonical_cov(qm.coverage()) == want, steps


def test_a_log_replay_ahead_of_a_growth_reads_its_own_batchs_lists(monkeypatch):
    """An index whose wide sites use the grouped log, a log of 64 words: every launch ends with entries to redo, and their replay
    runs at the head of the next launch — which is larger and swaps a fresh workspace in, retry lists included (the
    construction of test_log_replay's growth case). The replay must read the lists, the queues and the inputs of ITS batch:
    the oracle's coverage."""
    monkeypatch.setenv("GMX_DENSE_MAX_ALLELES", "2")
    ref = random_ref(6000, 11)
    prg, sites = mixed_variant_prg(ref, 150, 12, max_alleles=12)  # sites of more than 8 alleles among them
    reads = simulate_haplotype_reads(ref, sites, N, LEN, LEN, 13)
    seeds = master_seeds(42, [N])
    want = oracle_map(prg, 7, reads, seeds, threads=8)
    ix = Index(prg, 7)
    assert ix.uses_grouped_log
    flat = np.ascontiguousarray(np.asarray(reads, dtype=np.uint8)).reshape(N, LEN)
    qm = Quasimapper(ix, log_cap_words=64, max_batch_reads=1600)
    for lo, hi in ((0, 300), (300, 1500), (1500, 3000)):  # 300, 1200, 1500 reads: one launch each, each larger than the last
        qm.map_reads(flat[lo:hi].reshape(-1), flat_offsets(hi - lo, LEN), seeds[lo:hi])
    assert canonical_cov(qm.coverage()) == want
    assert qm.queue_counts()["log_replays"] > 0


@pytest.mark.parametrize("twobit", [False, True], ids=["planes", "2bit"])
def test_packed_feeds_go_round_the_slot_ring(snp_case, twobit):
    """max_batch_reads = 400: a call of 3000 reads is eight chunks through three slots. Three small calls size the slots small;
    the call from page-locked buffers then grows every one of them, the call from pageable buffers (registered for its
    duration) reuses them. Each gives the byte feed's coverage. A slot frees what it supersedes, so the engine ends owning
    what an engine given the large call alone owns — and, with the 2-bit stream, the one buffer of bit planes that the small
    calls unpacked into: the engine keeps a superseded plane buffer until it is destroyed."""
    ix, reads, seeds, want = snp_case
    pack = pack_reads_2bit if twobit else pack_reads
    offs = flat_offsets(N, LEN)
    qm = Quasimapper(ix, max_batch_reads=400)
    small = []
    for i in range(3):
        small.append(pack(reads[150 * i:150 * (i + 1)].reshape(-1), flat_offsets(150, LEN), uniform_len=LEN, pinned=True))
        qm.map_reads_packed(small[-1], np.ascontiguousarray(seeds[150 * i:150 * (i + 1)]))
    qm.sync()
    small_bytes = qm.debug_owned_bytes()
    for pinned in (True, False):
        pk = pack(reads.reshape(-1), offs, uniform_len=LEN, pinned=pinned)
        qm.reset()
        qm.map_reads_packed(pk, seeds)
        assert canonical_cov(qm.coverage()) == want, "pinned" if pinned else "pageable"
        pk.close()
    for pk in small:
        pk.close()
    alone = Quasimapper(ix, max_batch_reads=400)
    pk = pack(reads.reshape(-1), offs, uniform_len=LEN, pinned=True)
    alone.map_reads_packed(pk, seeds)
    assert canonical_cov(alone.coverage()) == want
    pk.close()
    kept = 8 * (150 * LEN // 32 + 150 + 16) if twobit else 0  # the planes of a 150-read launch (launch_batch: pairs of 8 bytes)
    print("owned bytes after the small calls:", small_bytes, "after the large ones:", qm.debug_owned_bytes(), "large call alone:", alone.debug_owned_bytes())
    assert small_bytes < qm.debug_owned_bytes() == alone.debug_owned_bytes() + kept


def test_a_failed_growth_leaves_the_engine_as_it_was(snp_case):
    """gmx_engine_reserve for 3000 reads on an engine sized by 500, with each host allocation of the call — the bookkeeping of
    the fresh workspace's and the engine's buffers — failing in turn (gmx_debug_fail_alloc, as test_alloc_failure walks a
    call): a negative code, the bytes owned before the call, and an engine that then maps the 3000 reads like a fresh one."""
    ix, reads, seeds, want = snp_case
    lib = _lib.load()
    qm, twin = Quasimapper(ix), Quasimapper(ix)
    for q in (qm, twin):
        _map_first(q, reads, seeds, 500)
    before = qm.debug_owned_bytes()
    grow = lambda q: lib.gmx_engine_reserve(q.h, N, N * LEN)
    n0 = lib.gmx_debug_fail_alloc(-1)  # count only: the allocations of the call, on an engine in the same state
    assert grow(twin) == 0
    n_allocs = lib.gmx_debug_fail_alloc(0) - n0
    assert n_allocs >= 1 and twin.debug_owned_bytes() > before
    for nth in range(1, n_allocs + 1):
        lib.gmx_debug_fail_alloc(nth)
        rc = grow(qm)
        lib.gmx_debug_fail_alloc(0)
        assert rc < 0 and lib.gmx_last_error(), (nth, rc)
        assert qm.debug_owned_bytes() == before, nth
    qm.reset()
    _map_first(qm, reads, seeds, N)
    assert canonical_cov(qm.coverage()) == want
    assert qm.debug_owned_bytes() == twin.debug_owned_bytes()  # (the engine whose reserve call went through)

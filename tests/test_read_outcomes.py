"""Per-read mapping outcomes (gmx_engine_record_outcomes, include/gmx.h): one byte per read — bits 0-1 the forward task's
code, 2-3 the reverse-complement task's (0 skipped, 1 missing k-mer, 2 no exact mapping, 3 exactly mapped), bit 4 / 5 "that
task's selection drew among more than one mapping instance". Compared read by read with the oracle, between the feeds, the
workspaces, the capacity tiers and the seed-screening routes, and with the five counters."""
import ctypes as C

import numpy as np
import pytest

from common import flatten_reads
from golden_runner import all_cases, prg_ints, seq
from oracle import Oracle
from gramtools_amd import Index, Quasimapper, master_seeds, pack_reads, pack_reads_2bit
from gramtools_amd.synth import (bracket_to_ints, nested_prg, random_ref, realistic_reads, simulate_graph_reads,
                                 simulate_snp_reads, snp_prg, split_reads)
from test_many_instances import tandem_prg, tandem_reads

pytestmark = pytest.mark.gpu

NAMES = ("skipped", "missing_kmer", "no_extension", "exact_mapped")


def fields(b):
    b = int(b)
    return b & 3, (b >> 2) & 3, (b >> 4) & 1, (b >> 5) & 1


def swapped(b):
    """The byte of the reverse complement of a read whose byte is b: task fields and multi bits change places."""
    f, r, mf, mr = fields(b)
    return r | (f << 2) | (mr << 4) | (mf << 5)


def check_counters(out, stats):
    """Identity with gmx_stats: the codes of all tasks add up to the four counters, all = 2 x reads."""
    out = np.asarray(out, dtype=np.uint8)
    assert not (out & 0xC0).any()
    codes = np.concatenate([out & 3, (out >> 2) & 3])
    for c, name in enumerate(NAMES):
        assert int((codes == c).sum()) == stats[name], (name, np.bincount(codes, minlength=4).tolist(), stats)
    assert stats["all"] == 2 * out.size


def oracle_task(o, k, read):
    """(code, multi) of ONE oriented read from the oracle's own steps (quasimap.cpp:159-194, coverage_common.cpp:95-141)."""
    read = np.asarray(read, dtype=np.uint8)
    if read.size < max(k, 1) or ((read < 1) | (read > 4)).any():
        return 0, 0
    states = o.search_read_backwards(read)
    if not states:
        return (2 if o.all_kmers_in_index(read) else 1), 0
    nonvar, entries = o.unique_site_paths(states)
    return 3, int(len(entries) > 0 and nonvar + len(entries) > 1)  # no class: no draw (coverage_common.cpp:96-97)


def oracle_bytes(prg, k, reads):
    """Every read mapped ALONE through Oracle.map_reads: its counters give the unordered pair of task codes. The
    orientation and the multi bits come from the oracle's search and selection steps on each oriented read; their pair
    must be the counters' pair."""
    o = Oracle(prg, k)
    out = np.zeros(len(reads), dtype=np.uint8)
    pairs = []
    before = o.stats()
    for i, r in enumerate(reads):
        r = np.asarray(r, dtype=np.uint8)
        if 0 < r.size < k:  # undefined in the reference (quasimap.cpp:206-210; the oracle refuses the read): skipped by definition
            assert oracle_task(o, k, r) == (0, 0)
            pairs.append([0, 0])
            continue
        o.map_reads(r if r.size else np.zeros(1, np.uint8), np.array([0, r.size], dtype=np.uint64), np.array([i + 1], dtype=np.uint32))
        after = o.stats()
        pair = sorted(c for c, name in enumerate(NAMES) for _ in range(after[name] - before[name]))
        assert len(pair) == 2 and after["all"] - before["all"] == 2
        before = after
        pairs.append(pair)
        (f, mf), (rv, mr) = oracle_task(o, k, r), oracle_task(o, k, o.reverse_complement(r) if r.size else r)
        assert sorted((f, rv)) == pair, (i, f, rv, pair)
        out[i] = f | (rv << 2) | (mf << 4) | (mr << 5)
    o.close()
    return out, pairs


def record(ix, reads, seeds=None, feed="bytes", chunk=0, **kw):
    """The outcome bytes, the coverage and the engine of `reads` through one feed, `chunk` reads per launch (0: all at once)."""
    qm = Quasimapper(ix, **kw)
    qm.record_outcomes(True)
    run_feed(qm, reads, seeds if seeds is not None else master_seeds(7, [len(reads)]), feed, chunk)
    return qm.outcomes(), qm.coverage(), qm


def run_feed(qm, reads, seeds, feed, chunk=0):
    n = len(reads)
    step = chunk or max(n, 1)
    keep = []
    for lo in range(0, n, step):
        part, s = reads[lo:lo + step], np.ascontiguousarray(seeds[lo:lo + step], dtype=np.uint32)
        flat, offs = flatten_reads(part)
        if feed == "bytes":
            qm.map_reads(flat, offs, s)
        elif feed == "packed":
            pk = pack_reads(flat, offs, pinned=True)
            qm.map_reads_packed(pk, s)
            keep.append(pk)
        elif feed == "2bit":
            pk = pack_reads_2bit(flat, offs, pinned=True)
            qm.map_reads_packed(pk, s)
            keep.append(pk)
        elif feed == "packed_device":
            import torch
            pk = pack_reads(flat, offs)
            dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (pk.planes, pk.offsets, s, pk.skip)]
            rc = qm.lib.gmx_map_reads_packed_device(qm.h, C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()), 0,
                                                    C.c_void_p(dev[2].data_ptr()), C.c_void_p(dev[3].data_ptr()), len(part))
            assert rc == 0, qm.lib.gmx_last_error()
            keep.append(dev)
        else:
            raise ValueError(feed)
    qm.sync()
    for pk in keep:
        if hasattr(pk, "close"):
            pk.close()


def check_against_oracle(prg, k, reads, **kw):
    want, _ = oracle_bytes(prg, k, reads)
    got, cov, qm = record(Index(prg, k), reads, **kw)
    assert qm.outcome_count() == len(reads)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(i), fields(got[i]), fields(want[i])) for i in bad[:10]]
    check_counters(got, cov.stats.as_dict())
    return got, want


def revcomp(r):
    return (5 - np.asarray(r, dtype=np.uint8))[::-1].copy()


def check_orientation(ix, reads, got):
    """The byte of revcomp(r) is the byte of r with the two task fields and the two multi bits swapped."""
    clean = [i for i, r in enumerate(reads) if len(r) and ((np.asarray(r) >= 1) & (np.asarray(r) <= 4)).all()]
    rc, _, _ = record(ix, [revcomp(reads[i]) for i in clean])
    assert [int(b) for b in rc] == [swapped(got[i]) for i in clean]


# ---- the cases -----------------------------------------------------------------------------------------------------
def flat_case():
    """2 kb, 20 SNPs, k = 5: 600 reads of 30-60 bases with substitutions, Ns and ragged ends, and reads of 1-4 bases."""
    ref = random_ref(2000, 3)
    prg, pos, alts, n_alts = snp_prg(ref, 20, 4)
    clean = simulate_snp_reads(ref, pos, alts, n_alts, 600, 60, 5)
    flat, offs = realistic_reads(clean, 6, sub_rate=0.01, n_read_frac=0.03, len_lo=30)
    reads = [np.array(r) for r in split_reads(flat, offs)]
    reads += [np.array(clean[i, :1 + i % 4]) for i in range(12)]
    return prg, 5, reads


def nested_case():
    prg = bracket_to_ints(nested_prg(41, n_top=10, max_depth=3).replace("t", "a"))
    return prg, 4, [np.asarray(r, dtype=np.uint8) for r in simulate_graph_reads(prg, 300, 16, 1)]


def repeat_case():
    """Ten tandem copies of a 60-base unit with a SNP site each, between unique flanks of 200: 200 reads of 30 bases from a
    haplotype, either strand. Inside the copies a read over the site has ten classes to draw from, one beside the site ten
    non-variant positions and no class (no draw); a read in the flanks has one mapping instance."""
    prg, unit, site_at, alt = tandem_prg(10, 60, 8, flank=200)
    rng = np.random.default_rng(9)
    ints = [int(x) for x in prg]
    hap, i = [], 0
    while i < len(ints):
        if ints[i] > 4:  # a site: [m, ref, m + 1, alt, m + 1]
            hap.append(ints[i + 1] if rng.random() < 0.5 else ints[i + 3])
            i += 5
        else:
            hap.append(ints[i])
            i += 1
    hap = np.asarray(hap, dtype=np.uint8)
    reads = []
    for j in range(200):
        st = int(rng.integers(0, hap.size - 30 + 1))
        r = hap[st:st + 30].copy()
        reads.append(revcomp(r) if j % 2 else r)
    return prg, 6, reads


def test_flat_prg_read_by_read_against_the_oracle():
    prg, k, reads = flat_case()
    got, want = check_against_oracle(prg, k, reads)
    codes = np.concatenate([want & 3, (want >> 2) & 3])
    assert all((codes == c).sum() > 10 for c in range(4)), np.bincount(codes, minlength=4)  # every code occurs
    check_orientation(Index(prg, k), reads, got)


def test_nested_prg_read_by_read_against_the_oracle():
    prg, k, reads = nested_case()
    got, want = check_against_oracle(prg, k, reads)
    check_orientation(Index(prg, k), reads, got)


def test_repeats_set_the_multi_bit_exactly_where_the_oracle_draws_among_several():
    prg, k, reads = repeat_case()
    got, want = check_against_oracle(prg, k, reads)
    multi = (want & 0x30) != 0
    mapped = ((want & 3) == 3) | (((want >> 2) & 3) == 3)
    assert multi.sum() > 20 and (mapped & ~multi).sum() > 20
    check_orientation(Index(prg, k), reads, got)
    # by construction: a read over the site inside the copies draws, a read in a unique flank does not
    _, unit, site_at, _ = tandem_prg(10, 60, 8, flank=200)
    inside = np.tile(unit, 2)[site_at - 10:site_at + 20]
    flank = np.asarray([int(x) for x in prg[20:50]], dtype=np.uint8)
    b, _, _ = record(Index(prg, k), [inside, flank])
    assert fields(b[0])[0] == 3 and fields(b[0])[2] == 1
    assert fields(b[1])[0] == 3 and fields(b[1])[2] == 0


def _golden_cases():
    out = []
    for f, c in all_cases():
        if f != "quasimap.json" or c.get("expect_build_error"):
            continue
        reads = []
        for op in c["ops"]:
            if op["op"] == "quasimap_read":
                reads.append(seq(op["read"]))
            elif op["op"] == "map_reads":
                reads += [seq(r) for r in op["reads"]]
        if reads and c["k"]:
            out.append((c["name"], prg_ints(c["prg"]), c["k"], reads))
    return out


def test_golden_prgs_read_by_read_against_the_oracle():
    cases = _golden_cases()
    assert len(cases) >= 5
    for name, prg, k, reads in cases:
        reads = [np.asarray(r, dtype=np.uint8) for r in reads]
        want, _ = oracle_bytes(prg, k, reads)
        got, cov, _ = record(Index(prg, k), reads)
        assert got.tolist() == want.tolist(), name
        check_counters(got, cov.stats.as_dict())


def test_a_read_of_the_prg_text_whose_reverse_complement_is_absent_maps_forward():
    prg = np.asarray([1, 1, 2, 1, 1, 3, 1, 1, 2, 2, 1, 1, 5, 2, 6, 3, 6, 1, 1, 2, 1, 3, 1, 1, 1], dtype=np.uint32)  # no T: no reverse complement maps
    read = np.asarray([1, 1, 2, 1, 1, 3, 1, 1, 2, 2], dtype=np.uint8)
    b, cov, _ = record(Index(prg, 3), [read, revcomp(read)])
    assert fields(b[0])[0] == 3 and fields(b[0])[1] in (1, 2)
    assert fields(b[1])[1] == 3 and fields(b[1])[0] in (1, 2)
    check_counters(b, cov.stats.as_dict())


# ---- feeds, workspaces, resets -------------------------------------------------------------------------------------
FEEDS = ("bytes", "packed", "2bit", "packed_device")


@pytest.mark.parametrize("twin", ["0", "1"])
def test_every_feed_gives_the_same_bytes(monkeypatch, twin):
    """All four feeds, whole and in launches of 97 reads (with GMX_TWIN=1 the two workspaces take them in turn: a launch's
    base read index is no multiple of four, words are shared between launches in flight), and across a queued reset."""
    import torch
    monkeypatch.setenv("GMX_TWIN", twin)
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    want, cov, _ = record(ix, reads, seeds)
    check_counters(want, cov.stats.as_dict())
    for feed in FEEDS:
        for chunk in (0, 97):
            got, cov2, qm = record(ix, reads, seeds, feed=feed, chunk=chunk)
            assert bool(qm.lib.gmx_engine_second_stream(qm.h)) == (twin == "1")  # (the engine really has two workspaces)
            assert got.tolist() == want.tolist(), (feed, chunk)
            assert cov2.stats.as_dict() == cov.stats.as_dict()
            if chunk:  # a queued reset: the count starts again, nothing of the reads before shows
                qm.reset(stream=torch.cuda.current_stream().cuda_stream)
                assert qm.outcome_count() == 0
                run_feed(qm, reads[100:], seeds[100:], feed, chunk)
                assert qm.outcome_count() == len(reads) - 100
                assert qm.outcomes().tolist() == want[100:].tolist(), (feed, "after reset")
                assert qm.outcomes(5, 40).tolist() == want[105:145].tolist()
                check_counters(qm.outcomes(), qm.coverage().stats.as_dict())
                qm.reset()
                assert qm.outcome_count() == 0
                run_feed(qm, reads[:50], seeds[:50], feed, chunk)
                assert qm.outcomes().tolist() == want[:50].tolist()


def tiled(reads, seeds, copies):
    """(flat, offsets, seeds) of one launch: `copies` copies of the reads back to back, put together with numpy."""
    flat, offs = flatten_reads(reads)
    ends = np.cumsum(np.tile(np.diff(offs.astype(np.int64)), copies))
    return np.tile(flat, copies), np.concatenate([[0], ends]).astype(np.uint64), np.tile(np.asarray(seeds, dtype=np.uint32), copies)


def test_a_full_buffer_grows_and_carries_the_recorded_bytes_over(monkeypatch):
    """The buffer starts at 1 MiB. Four launches of 430 copies of the first 611 reads of the flat case, 262 730 reads each: the fourth
    needs 1 050 920 bytes and makes the buffer grow with 788 190 bytes recorded — no multiple of 4, and 611 is odd: the launches
    share words, the carry-over is rounded to whole words. With GMX_TWIN=1 the launch before may still be in flight on the other
    workspace. Every byte is the oracle's for its read (which depends on the read alone); a reset clears the grown buffer."""
    monkeypatch.setenv("GMX_TWIN", "1")
    prg, k, reads = flat_case()
    reads = reads[:611]
    seeds = master_seeds(7, [len(reads)])
    want, _ = oracle_bytes(prg, k, reads)
    copies, launches = 430, 4
    per_launch = copies * len(reads)
    assert (launches - 1) * per_launch < (1 << 20) < launches * per_launch and ((launches - 1) * per_launch) % 4
    flat, offs, s = tiled(reads, seeds, copies)
    qm = Quasimapper(Index(prg, k))
    qm.record_outcomes(True)
    assert qm.lib.gmx_engine_second_stream(qm.h)
    for _ in range(launches):
        qm.map_reads(flat, offs, s)
    qm.sync()
    assert qm.outcome_count() == launches * per_launch
    got = qm.outcomes()
    bad = np.flatnonzero(got != np.tile(want, launches * copies))
    assert got.shape == (launches * per_launch,) and bad.size == 0, [(int(i), fields(got[i]), fields(want[i % len(reads)])) for i in bad[:10]]
    qm.reset()  # the grown buffer is cleared over its used prefix
    one_flat, one_offs = flatten_reads(reads)
    qm.map_reads(one_flat, one_offs, seeds)
    assert qm.outcome_count() == len(reads)
    assert qm.outcomes().tolist() == want.tolist()


def test_recording_off_leaves_nothing_and_changes_nothing():
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    flat, offs = flatten_reads(reads)
    off = Quasimapper(ix)
    off.map_reads(flat, offs, seeds)
    assert off.outcome_count() == 0
    a = off.coverage()
    _, b, _ = record(ix, reads, seeds)
    assert (a.raw_allele_sum == b.raw_allele_sum).all() and (a.raw_per_base == b.raw_per_base).all()
    assert (a.raw_grouped == b.raw_grouped).all() and a.stats.as_dict() == b.stats.as_dict()
    on_off = Quasimapper(ix)  # switched off again: later calls append nothing
    on_off.record_outcomes(True)
    on_off.map_reads(flat, offs, seeds)
    on_off.record_outcomes(False)
    on_off.map_reads(flat, offs, seeds)
    assert on_off.outcome_count() == len(reads)


# ---- capacity tiers, seed screening --------------------------------------------------------------------------------
def test_every_tier_leaves_the_bytes_of_the_default_capacities():
    """300 tandem copies: with the default pools the large-capacity pass holds the reads' 300 mapping instances; with small
    ones the tasks pass the 16-lane split search and the one-lane large slot, overflow both, and end in the heap-backed
    tier. One code per task either way."""
    prg, unit, site_at, alt = tandem_prg(300, 60, 5)
    reads = tandem_reads(unit, site_at, alt, 100, 6)
    reads += [np.asarray(r[:40]) for r in reads[:3]] + [np.asarray([int(x) for x in prg[3:33]], dtype=np.uint8)]
    ix = Index(prg, 8)
    want, _ = oracle_bytes(prg, 8, reads)
    big, cov, qm = record(ix, reads)
    counts = qm.queue_counts()
    assert counts["big_mapped"] + counts["inst_mapped"] + counts["cover_overflow"] > 0 and counts["huge_search"] + counts["huge_cover"] == 0
    assert big.tolist() == want.tolist()
    check_counters(big, cov.stats.as_dict())
    small, cov2, qm2 = record(ix, reads, max_states=64, max_path_nodes=128)
    counts2 = qm2.queue_counts()
    # every tier ran: the tasks entered the 16-lane split search (the overflow queues it serves), a lane's share of a slot did
    # not suffice (overflow_split: redone by one lane with a whole slot), nor did the slot (huge_search: the heap-backed tier)
    assert counts2["overflow_probe"] + counts2["overflow_extend"] >= 4, counts2
    assert counts2["overflow_split"] >= 4, counts2
    assert counts2["huge_search"] >= 4, counts2
    assert small.tolist() == big.tolist()
    check_counters(small, cov2.stats.as_dict())
    assert (cov.raw_allele_sum == cov2.raw_allele_sum).all()


@pytest.mark.parametrize("k,shift", [(5, "0"), (4, "2")])
def test_seed_cursor_with_and_without_the_side_table(monkeypatch, k, shift):
    """The seed cursor forced on (every multi-state entry taken state by state, screened through the side table or — with
    GMX_NO_SEED_SIDE=1 — by the header walk), entries addressed in units: the same bytes, and the oracle's."""
    prg = bracket_to_ints(nested_prg(43, n_top=10, max_depth=3).replace("t", "a"))
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_graph_reads(prg, 200, 16, 2)]
    reads += [np.asarray(r[:9]) for r in reads[:20]]
    want, _ = oracle_bytes(prg, k, reads)
    monkeypatch.setenv("GMX_SEED_SHIFT", shift)
    monkeypatch.setenv("GMX_SEED_CURSOR", "1")
    ix = Index(prg, k)
    for no_side in (False, True):
        if no_side:
            monkeypatch.setenv("GMX_NO_SEED_SIDE", "1")
        got, cov, qm = record(ix, reads)
        assert qm.queue_counts()["seed_cursor"] == 1
        assert got.tolist() == want.tolist(), "header walk" if no_side else "side table"
        check_counters(got, cov.stats.as_dict())


# ---- forward-only engines, the grouped log, engine groups ----------------------------------------------------------
def test_forward_only_engine_leaves_the_reverse_fields_empty():
    prg, k, reads = flat_case()
    want, _ = oracle_bytes(prg, k, reads)
    got, cov, _ = record(Index(prg, k), reads, forward_only=True)
    assert got.tolist() == (want & 0x13).tolist()  # the forward code and its multi bit; nothing for the orientation not mapped
    st = cov.stats.as_dict()
    assert st["all"] == len(reads)
    codes = got & 3
    for c, name in enumerate(NAMES):
        assert int((codes == c).sum()) == st[name], name


def test_sites_on_the_grouped_log_and_its_replay():
    """Sites with more than 8 alleles record their grouped counts in the log; with a tiny log the tasks that find it full are
    redone after a drain (log replay). The bytes are those of a roomy log, and the oracle's."""
    from gramtools_amd.synth import mixed_variant_prg, simulate_haplotype_reads
    ref = random_ref(3000, 5)
    prg, sites = mixed_variant_prg(ref, 60, 6, max_alleles=12)
    reads = [np.asarray(r, dtype=np.uint8) for r in simulate_haplotype_reads(ref, sites, 600, 40, 80, 7)]
    ix = Index(prg, 6)
    want, _ = oracle_bytes(prg, 6, reads)
    roomy, cov, _ = record(ix, reads)
    assert roomy.tolist() == want.tolist()
    check_counters(roomy, cov.stats.as_dict())
    tiny, cov2, qm = record(ix, reads, chunk=150, log_cap_words=64)
    assert qm.queue_counts()["log_replays"] > 0
    assert tiny.tolist() == want.tolist()
    check_counters(tiny, cov2.stats.as_dict())
    assert cov2.grouped_allele_counts == cov.grouped_allele_counts


def test_a_group_puts_its_engines_ranges_together_in_read_order():
    """Two and three engines on one device: every feed call deals contiguous ranges of its reads; gmx_group_fetch_outcomes
    returns the bytes in the order the reads were handed over, over several calls, sub-ranges included, and starts again
    after a reset of the engines."""
    from gramtools_amd import QuasimapperGroup
    prg, k, reads = flat_case()
    ix = Index(prg, k)
    seeds = master_seeds(3, [len(reads)])
    want, _, _ = record(ix, reads, seeds)
    for devices in ([0, 0], [0, 0, 0]):
        grp = QuasimapperGroup(ix, devices)
        assert grp.outcome_count() == 0
        grp.record_outcomes(True)
        cuts = [0, 101, 350, len(reads)]
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            flat, offs = flatten_reads(reads[lo:hi])
            if j == 1:
                pk = pack_reads(flat, offs, pinned=True)
                grp.map_reads_packed(pk, seeds[lo:hi])
            else:
                grp.map_reads(flat, offs, seeds[lo:hi])
        assert grp.outcome_count() == len(reads)
        assert grp.outcomes().tolist() == want.tolist(), devices
        assert grp.outcomes(97, 300).tolist() == want[97:397].tolist()
        grp.allreduce()
        check_counters(grp.outcomes(), grp.coverage().stats.as_dict())
        assert grp.outcomes().tolist() == want.tolist()  # (the exchange leaves the bytes alone)
        for i in range(len(devices)):
            assert grp.lib.gmx_engine_reset(C.c_void_p(grp.lib.gmx_group_engine(grp.h, i))) == 0
        assert grp.outcome_count() == 0
        flat, offs = flatten_reads(reads[200:])
        grp.map_reads(flat, offs, seeds[200:])
        assert grp.outcomes().tolist() == want[200:].tolist()
        pk.close()
        grp.close()


# ---- gram genotype --read_outcomes ----------------------------------------------------------------------------------
COV_FILES = ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")


def parse_outcomes_file(data: bytes):
    """read_outcomes.bin: "GMXO", uint32 version, uint64 read count (little-endian), then one byte per read."""
    import struct
    magic, version, n = struct.unpack_from("<4sIQ", data, 0)
    assert magic == b"GMXO" and version == 1 and len(data) == 16 + n, (magic, version, n, len(data))
    return np.frombuffer(data, dtype=np.uint8, offset=16)


@pytest.fixture(scope="module")
def cli_sample(tmp_path_factory):
    """About 7 000 ragged reads of up to 60 bases with Ns in every form `gram` reads, the run without the flag, and the bytes the
    engine itself gives for these reads."""
    import gzip
    from bam_common import bam_bytes, record as bam_record, reverse_complement
    from ingest_formats_common import fasta_text, gram
    from test_ingest import bgzf
    d = tmp_path_factory.mktemp("outcomes_cli")
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
    (d / "s.plain.fq.gz").write_bytes(gzip.compress(fq, 6))
    (d / "s.fa").write_bytes(fasta_text(txt, 50))
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
    want, _, _ = record(Index(prg, 6), enc)
    return dict(run=run, cov=[(plain_out / "coverage" / f).read_bytes() for f in COV_FILES], want=want, noflag=plain_out)


CLI_FORMS = [("plain-one-thread", "s.fq", {}, ["--max_threads", "1"]),
             ("plain-host-parser", "s.fq", {"GMX_HOST_FASTQ": "1"}, []),
             ("bgzf", "s.bgzf.fq.gz", {}, []),
             ("gzip", "s.plain.fq.gz", {}, []),
             ("fasta", "s.fa", {}, []),
             ("bam", "s.bam", {}, []),
             ("two-engines", "s.fq", {"GMX_TEXT_CHUNK": "30000"}, ["--devices", "0,0"]),
             ("two-engines-host-parser", "s.fq", {"GMX_HOST_FASTQ": "1"}, ["--devices", "0,0"]),
             ("takeover", "s.bgzf.fq.gz", {"GMX_INGEST_MEMBERS": "20", "GMX_INGEST_TEST_FAIL_CHUNK": "2", "GMX_FASTQ_BLOCK": "200000"}, []),
             ("takeover-two-engines", "s.fq", {"GMX_TEXT_CHUNK": "30000", "GMX_INGEST_TEST_FAIL_CHUNK": "3"}, ["--devices", "0,0"])]


@pytest.mark.parametrize("name,reads_file,env,extra", CLI_FORMS, ids=[f[0] for f in CLI_FORMS])
def test_gram_read_outcomes_on_every_route(cli_sample, name, reads_file, env, extra):
    """Every form of the sample gives the SAME read_outcomes.bin — the bytes the engine gives for these reads in file order —,
    json counts equal to the printed counters, and the three coverage files of a run without the flag."""
    import json
    out, stdout = cli_sample["run"](name, reads_file, env, ["--read_outcomes", *extra])
    if name.startswith("takeover"):
        assert "the host reader takes over" in stdout and "gave up after 0 reads" not in stdout, stdout
    got = parse_outcomes_file((out / "read_outcomes.bin").read_bytes())
    assert got.size == 7300
    assert got.tolist() == cli_sample["want"].tolist()
    counters = [int(l.rsplit(":", 1)[1]) for l in stdout.splitlines() if l.startswith("Count ")]
    assert len(counters) == 5
    js = json.loads((out / "read_outcomes.json").read_text())
    assert js["reads"] == 7300 and counters[0] == 2 * 7300
    assert [js["tasks"][n] for n in NAMES] == counters[1:]
    assert {int(v): c for v, c in js["bytes"].items()} == {int(v): int(c) for v, c in zip(*np.unique(got, return_counts=True))}
    assert [(out / "coverage" / f).read_bytes() for f in COV_FILES] == cli_sample["cov"]
    assert not (cli_sample["noflag"] / "read_outcomes.bin").exists()

"""Strand evidence in the calls, host side (no GPU): gmx_strand_bias_phred against exact arithmetic, gmx_infer_annotate_strands
on hand-made per-strand grouped counts, and the log exchange's merge (gmx_grouped_log_merge_gathered) with records that carry
GMX_LOG_REVERSE. strand_bias_common.py holds what the GPU tests (test_strand_log.py) share with these."""
import ctypes as C
import gzip
import itertools
import math

import numpy as np
import pytest

from gramtools_amd import Coverage, Genotyped, Index, QuasimapReadsStats, _lib
from gramtools_amd.quasimap import GROUPED_LOG, LOG_COUNTED, LOG_REVERSE
from gramtools_amd.synth import bracket_to_ints, nested_prg
from strand_bias_common import (counted, exact_phred, expected_fields, strip_json, strip_vcf)

GMX_EINVAL = -1


# ---- H1: the score ---------------------------------------------------------------------------------------------------
BIG_TABLES = [(50, 50, 50, 50), (100, 0, 0, 100), (30, 2, 3, 29), (65535, 65535, 1, 0), (1, 0, 65535, 65535), (70000, 3, 5, 70000)]


def check_table(lib, t):
    a, b, c, d = t
    got = lib.gmx_strand_bias_phred(a, b, c, d)
    want = exact_phred(a, b, c, d)
    assert abs(got - want) <= 1e-6, (t, got, want)
    assert got >= 0.0 and not math.isnan(got) and math.copysign(1.0, got) == 1.0, (t, got)
    assert lib.gmx_strand_bias_phred(a, c, b, d) == pytest.approx(got, abs=1e-9), ("transposed", t)
    assert lib.gmx_strand_bias_phred(c, d, a, b) == pytest.approx(got, abs=1e-9), ("rows swapped", t)
    return got


def test_the_score_of_every_small_table_is_the_exact_fisher_probability():
    lib = _lib.load()
    n_zero = 0
    for t in itertools.product(range(7), repeat=4):
        got = check_table(lib, t)
        a, b, c, d = t
        if 0 in (a + b, c + d, a + c, b + d):
            assert got == 0.0, t
            n_zero += 1
    assert n_zero > 0
    assert lib.gmx_strand_bias_phred(3, 3, 3, 3) == 0.0            # p = 1
    assert lib.gmx_strand_bias_phred(6, 0, 0, 6) == pytest.approx(-10 * math.log10(2 / math.comb(12, 6)), abs=1e-9)  # the tie: both corners


@pytest.mark.parametrize("t", BIG_TABLES, ids=[",".join(map(str, t)) for t in BIG_TABLES])
def test_the_score_of_large_tables(t):
    got = check_table(_lib.load(), t)
    if t == (50, 50, 50, 50):
        assert got == 0.0
    if t == (70000, 3, 5, 70000):
        assert got > 100000  # far below the smallest double as a probability: the score is still finite
        assert math.isfinite(got)


# ---- H2: the annotation on hand-made counts --------------------------------------------------------------------------
NINE = ["AAA", "AAC", "AAG", "ACA", "ACC", "ACG", "AGA", "AGC", "AGG"]


def flat_prg():
    """Three sites: 2 alleles (A | C), 3 alleles (A | C | G) and 9 alleles of three bases (on the grouped log)."""
    enc = lambda s: ["ACGT".index(ch) + 1 for ch in s]
    ints = enc("GATTACAGATTC") + [5] + enc("A") + [6] + enc("C") + [6] + enc("TTGACCATGACA") + [7] + enc("A") + [8] + enc("C") + [8] + enc("G") + [8]
    ints += enc("CTAGGATCCTAT") + [9]
    for al in NINE:
        ints += enc(al) + [10]
    ints += enc("TGCATGCATTGA")
    return np.asarray(ints, dtype=np.uint32)


class Case:
    """Per-strand grouped counts of every site, written as the engine would return them: dense slots, counted log records."""

    def __init__(self, ix, fwd, rev):
        self.ix, self.groups = ix, (fwd, rev)
        n_slots = max(ix.info.n_grouped_slots, 1)
        self.dense = [np.zeros(n_slots, dtype=np.uint32) for _ in (0, 1)]
        self.logs = [[], []]
        for st in (0, 1):
            for s, gp in enumerate(self.groups[st]):
                for ids, count in gp.items():
                    if int(ix.grouped_off[s]) == GROUPED_LOG:
                        self.logs[st] += counted(s, ids, count)
                    else:
                        self.dense[st][int(ix.grouped_off[s]) + sum(1 << a for a in ids) - 1] += count
        self.logs = [np.asarray(l, dtype=np.uint32) for l in self.logs]
        # per-base coverage of an allele's bases: its haploid coverage (both strands)
        pb = np.zeros(max(ix.info.n_per_base_slots, 1), dtype=np.uint32)
        for s, al, _, off, ln in ix.per_base_layout():
            pb[off:off + ln] = sum(c for st in (0, 1) for ids, c in self.groups[st][s].items() if int(al) in ids)
        self.pb = pb[:ix.info.n_per_base_slots]
        stats = QuasimapReadsStats(0, 0, 0, 0, 0)
        zeros = np.zeros(ix.info.n_allele_slots, dtype=np.uint32)
        self.strand = [Coverage(ix, zeros, self.pb, self.dense[st][:ix.info.n_grouped_slots], self.logs[st], stats) for st in (0, 1)]
        total_log = np.concatenate(self.logs) if sum(l.size for l in self.logs) else np.zeros(0, dtype=np.uint32)
        self.total = Coverage(ix, zeros, self.pb, (self.dense[0] + self.dense[1])[:ix.info.n_grouped_slots], total_log, stats)

    def genotyped(self, ploidy="haploid", annotate=True):
        g = Genotyped(self.total, 0.001, ploidy, depth=dict(mean=20.0, variance=25.0))
        if annotate:
            g.annotate_strands(self.strand[0], self.strand[1])
        return g


def check_sites(case, g, hapg_of):
    """Every site's three fields against the definitions, restated from what the site reports (strand_bias_common.expected_fields).
    hapg_of(site index, site json) -> the haplogroup of every output allele, or None where the test cannot know it."""
    sites = [g.site(i) for i in range(case.ix.n_sites)]
    for i, s in enumerate(sites):
        if s["GT"][0][0] is None:
            assert s["COV_FWD"] == [[]] and s["COV_REV"] == [[]] and s["SB"] == [None], (i, s)
            continue
        want = expected_fields(s, case.groups[0][i], case.groups[1][i], hapg_of(i, s))
        for key in ("COV_FWD", "COV_REV"):
            assert len(s[key][0]) == len(s["ALS"])
            for got, w in zip(s[key][0], want[key]):
                assert w is None or got == w, (i, key, s, want)
        assert abs(s["SB"][0] - want["SB"]) <= 1e-6, (i, s, want)
    return sites


@pytest.fixture(scope="module")
def flat_ix():
    ix = Index(flat_prg(), 5, threads=1)
    assert [int(n) for n in ix.n_alleles] == [2, 3, 9] and [int(o) == GROUPED_LOG for o in ix.grouped_off] == [False, False, True]
    return ix


def flat_hapg(i, s):
    seqs = [["A", "C"], ["A", "C", "G"], NINE][i]
    return [seqs.index(a) for a in s["ALS"]]


def test_balanced_strands_score_zero(flat_ix):
    gp = [{(0,): 2, (1,): 20}, {(2,): 18, (0,): 2, (0, 1): 2}, {(4,): 20, (1,): 2, (1, 7): 2}]
    case = Case(flat_ix, gp, gp)
    sites = check_sites(case, case.genotyped(), flat_hapg)
    assert [s["HAPG"] for s in sites] == [[[1]], [[2]], [[4]]]
    assert all(s["SB"] == [0.0] for s in sites)
    assert sites[0]["COV_FWD"] == sites[0]["COV_REV"] == [[2, 20]]
    assert sites[2]["ALS"] == ["AAA", "ACC"] and sites[2]["COV_FWD"] == [[0, 20]]


def test_a_call_seen_on_one_strand_only(flat_ix):
    """The called allele on the forward strand only, the rest on both; at the log site too."""
    fwd = [{(0,): 3, (1,): 40}, {(2,): 36, (0,): 3, (1,): 2}, {(4,): 40, (1,): 3, (8,): 2}]
    rev = [{(0,): 3}, {(0,): 3, (1,): 2}, {(1,): 3, (8,): 2}]
    case = Case(flat_ix, fwd, rev)
    sites = check_sites(case, case.genotyped(), flat_hapg)
    assert [s["HAPG"] for s in sites] == [[[1]], [[2]], [[4]]]
    assert sites[0]["COV_FWD"] == [[3, 40]] and sites[0]["COV_REV"] == [[3, 0]]
    assert sites[2]["COV_FWD"] == [[0, 40]] and sites[2]["COV_REV"] == [[0, 0]]
    assert all(s["SB"][0] > 20 for s in sites)
    # the reverse arrays all zero: one margin of every table is zero
    empty = [dict() for _ in range(3)]
    case = Case(flat_ix, fwd, empty)
    sites = check_sites(case, case.genotyped(), flat_hapg)
    assert all(s["SB"] == [0.0] and not any(s["COV_REV"][0]) for s in sites) and sites[1]["COV_FWD"] == [[3, 36]]


def test_a_group_shared_with_the_called_haplogroup_counts_as_called(flat_ix):
    fwd = [{(1,): 20, (0, 1): 15, (0,): 1}, {(2,): 20, (1, 2): 15, (1,): 1}, {(4,): 20, (4, 6): 15, (6,): 1}]
    rev = [{(1,): 20, (0,): 9}, {(2,): 20, (1,): 9}, {(4,): 20, (6,): 9}]
    case = Case(flat_ix, fwd, rev)
    sites = check_sites(case, case.genotyped(), flat_hapg)
    assert [s["HAPG"] for s in sites] == [[[1]], [[2]], [[4]]]
    lib = _lib.load()
    for s in sites:  # called 35 / 20, other 1 / 9 — not 20 / 20 and 16 / 9
        assert s["SB"][0] == pytest.approx(lib.gmx_strand_bias_phred(35, 20, 1, 9), abs=1e-12)
        assert abs(s["SB"][0] - lib.gmx_strand_bias_phred(20, 20, 16, 9)) > 1e-3
    assert sites[0]["COV_FWD"] == [[16, 35]] and sites[2]["COV_FWD"] == [[0, 35]]


def test_a_null_site_has_no_fields_and_a_heterozygous_call_has_two_haplogroups(flat_ix):
    fwd = [dict(), {(0,): 14, (2,): 4, (1,): 3}, {(2,): 12, (5,): 3, (0,): 2}]
    rev = [dict(), {(0,): 2, (2,): 15, (1,): 1}, {(2,): 1, (5,): 11, (0,): 4}]
    case = Case(flat_ix, fwd, rev)
    g = case.genotyped("diploid")
    sites = check_sites(case, g, flat_hapg)
    assert sites[0]["GT"] == [[None]] and sites[0]["SB"] == [None]
    assert sites[1]["GT"] == [[0, 1]] and sites[1]["ALS"] == ["A", "G"] and sites[1]["HAPG"] == [[0, 2]] and sites[2]["HAPG"] == [[2, 5]]
    lib = _lib.load()
    assert sites[1]["SB"][0] == pytest.approx(lib.gmx_strand_bias_phred(18, 17, 3, 1), abs=1e-12)
    assert sites[2]["SB"][0] == pytest.approx(lib.gmx_strand_bias_phred(15, 12, 2, 4), abs=1e-12)


def test_counts_beyond_16_bits_are_not_wrapped(flat_ix):
    """The model's counters are 16 bits wide (the totals wrap); the strand fields are the raw sums."""
    fwd = [{(1,): 70000, (0,): 3}, dict(), {(3,): 70000, (0,): 3}]
    rev = [{(1,): 5, (0,): 70000}, dict(), {(3,): 5, (0,): 70000}]
    case = Case(flat_ix, fwd, rev)
    sites = check_sites(case, case.genotyped(), flat_hapg)
    called = [s for s in (sites[0], sites[2]) if s["GT"][0][0] is not None]
    assert called
    for s in called:
        assert s["COV_FWD"][0][0] == 3 and s["COV_REV"][0][0] == 70000
        if len(s["ALS"]) > 1:
            assert s["COV_FWD"][0][1] == 70000 and s["COV_REV"][0][1] == 5
        assert s["SB"][0] > 100000


def test_nested_sites_use_their_own_counts_and_calls():
    prg = bracket_to_ints(nested_prg(71, n_top=8, max_depth=3))
    ix = Index(prg, 4, threads=1)
    assert ix.is_nested
    rng = np.random.default_rng(9)
    fwd, rev = [], []
    for s in range(ix.n_sites):
        n = int(ix.n_alleles[s])
        call = int(rng.integers(0, n))
        other = (call + 1) % n
        fwd.append({(call,): int(rng.integers(15, 30)), (other,): int(rng.integers(0, 4)), tuple(sorted((call, other))): 2})
        rev.append({(call,): int(rng.integers(0, 30)), (other,): int(rng.integers(0, 4))})
        fwd[-1] = {k: v for k, v in fwd[-1].items() if v}
        rev[-1] = {k: v for k, v in rev[-1].items() if v}
    case = Case(ix, fwd, rev)

    def hapg_of(i, s):  # the called alleles' haplogroups are reported; the reference allele is the first path
        known = [None] * len(s["ALS"])
        known[0] = 0
        for gt, h in zip(s["GT"][0], s["HAPG"][0]):
            known[gt] = h
        return known

    sites = check_sites(case, case.genotyped(), hapg_of)
    called = [s for s in sites if s["GT"][0][0] is not None]
    assert len(called) >= 3 and any(int(ix.parent_site[i]) != 0 for i, s in enumerate(sites) if s["GT"][0][0] is not None)
    assert len({s["SB"][0] for s in called}) > 1


def test_the_files_gain_the_three_fields_and_nothing_else(flat_ix, tmp_path):
    fwd = [dict(), {(0,): 14, (2,): 4, (1,): 3}, {(2,): 12, (5,): 3, (0,): 2}]
    rev = [dict(), {(0,): 2, (2,): 15, (1,): 1}, {(2,): 1, (5,): 11, (0,): 4}]
    case = Case(flat_ix, fwd, rev)
    files = {}
    for name, annotate in (("plain", False), ("strands", True)):
        d = tmp_path / name
        d.mkdir()
        case.genotyped("diploid", annotate).write(str(d), "s1")
        files[name] = ((d / "genotyped.json").read_text(), gzip.decompress((d / "genotyped.vcf.gz").read_bytes()).decode(),
                       (d / "personalised_reference.fasta").read_bytes())
    plain, strands = files["plain"], files["strands"]
    for text in plain[:2]:
        assert "COV_FWD" not in text and "COV_REV" not in text and "SB" not in text
    assert strip_json(strands[0]) == plain[0] and strands[0] != plain[0]
    assert strip_vcf(strands[1]) == plain[1] and strands[1] != plain[1]
    assert strands[2] == plain[2]
    import json
    j = json.loads(strands[0])
    assert list(j["Site_Fields"]) == sorted(j["Site_Fields"]) and {"COV_FWD", "COV_REV", "SB"} <= set(j["Site_Fields"])
    assert all(list(s) == sorted(s) for s in j["Sites"])  # keys stay in alphabetical order
    assert j["Sites"][0]["SB"] == [None] and j["Sites"][1]["COV_FWD"] == [[14, 4]] and j["Sites"][1]["COV_REV"] == [[2, 15]]
    lines = strands[1].splitlines()
    head = [l for l in lines if l.startswith("##FORMAT")]
    assert [l.split(",")[0] for l in head[-3:]] == ["##FORMAT=<ID=COV_FWD", "##FORMAT=<ID=COV_REV", "##FORMAT=<ID=SB"]
    assert "Number=R,Type=Integer" in head[-3] and "Number=R,Type=Integer" in head[-2] and "Number=1,Type=Float" in head[-1]
    recs = [l.split("\t") for l in lines if not l.startswith("#")]
    assert all(r[8].endswith(":GT_CONF:GT_CONF_PERCENTILE:COV_FWD:COV_REV:SB") for r in recs)
    assert recs[0][9].endswith(":.:.:.") and recs[0][9].startswith(".:")
    f = dict(zip(recs[1][8].split(":"), recs[1][9].split(":")))
    assert f["COV_FWD"] == "14,4" and f["COV_REV"] == "2,15" and float(f["SB"]) == pytest.approx(j["Sites"][1]["SB"][0], rel=1e-5)


def test_annotate_refuses_what_it_cannot_read(flat_ix):
    case = Case(flat_ix, [dict(), dict(), {(2,): 3}], [dict(), dict(), {(2,): 3}])
    g = case.genotyped(annotate=False)
    lib = _lib.load()
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    dense = np.zeros(flat_ix.info.n_grouped_slots, dtype=np.uint32)
    assert lib.gmx_infer_annotate_strands(None, u32(dense), u32(dense), None, 0, None, 0) == GMX_EINVAL
    assert lib.gmx_infer_annotate_strands(g.h, None, u32(dense), None, 0, None, 0) == GMX_EINVAL
    for bad in ([2, 1 | LOG_REVERSE, 3], [7, 1, 3], [2, 1, 9], [2, 3 | LOG_COUNTED, 1, 0, 4]):  # strand bit, site, allele id, cut short
        rec = np.asarray(bad, dtype=np.uint32)
        assert lib.gmx_infer_annotate_strands(g.h, u32(dense), u32(dense), u32(rec), rec.size, None, 0) == GMX_EINVAL, bad
    assert "SB" not in g.site(2)


# ---- H3: the merge of gathered logs ----------------------------------------------------------------------------------
def merge(slices):
    lib = _lib.load()
    pad = max([len(s) for s in slices] + [1])
    gathered = np.zeros(len(slices) * pad, dtype=np.uint32)
    for r, s in enumerate(slices):
        gathered[r * pad:r * pad + len(s)] = s
    sizes = np.asarray([len(s) for s in slices], dtype=np.uint64)
    n = lib.gmx_grouped_log_merge_gathered(gathered.ctypes.data, sizes.ctypes.data, len(slices), pad, None, 0)
    assert n >= 0
    out = np.zeros(max(n, 1), dtype=np.uint32)
    assert lib.gmx_grouped_log_merge_gathered(gathered.ctypes.data, sizes.ctypes.data, len(slices), pad, out.ctypes.data, n) == n
    return [int(x) for x in out[:n]]


R, K = LOG_REVERSE, LOG_COUNTED


def test_merge_without_the_strand_bit_is_what_it_was():
    # world 2, both record forms, a pad word: the literal is what the function returned before it knew the bit
    got = merge([[3, 2, 1, 4, 0xFFFFFFFF, 3, 2 | K, 5, 0, 1, 4, 0, 1, 7], [0, 1, 7, 3, 1, 2]])
    assert got == [0, 1 | K, 2, 0, 7, 3, 2 | K, 6, 0, 1, 4, 3, 1 | K, 1, 0, 2]  # (key order: [3, 1, 4] before [3, 2])
    assert merge([[], [3, 2, 1, 4], []]) == [3, 2 | K, 1, 0, 1, 4]  # world 3, two empty ranks
    assert merge([[], []]) == []


@pytest.mark.parametrize("world", [2, 3])
def test_merge_keeps_the_strands_apart(world):
    a = [3, 2, 1, 4, 3, 2 | R, 1, 4, 3, 2 | R, 1, 4]                                  # plain form: forward once, reverse twice
    b = [3, 2 | K | R, 5, 0, 1, 4, 3, 2 | K, 7, 1, 1, 4, 0, 1 | K | R, 2, 0, 6]    # counted form; site 0 on the reverse strand only
    slices = [a, [], b][:world] if world == 3 else [a, b]
    got = merge(slices)
    want = [0, 1 | K | R, 2, 0, 6, 3, 2 | K, 8, 1, 1, 4, 3, 2 | K | R, 7, 0, 1, 4]  # a key's forward record, then its reverse one
    assert got == want
    assert merge([got, []]) == got  # merged output is valid input


def test_merge_reads_the_id_count_without_both_flags():
    lib = _lib.load()
    cut = np.asarray([3, 2 | K | R, 5, 0, 1], dtype=np.uint32)  # two ids announced, one present
    sizes = np.asarray([cut.size], dtype=np.uint64)
    assert lib.gmx_grouped_log_merge_gathered(cut.ctypes.data, sizes.ctypes.data, 1, cut.size, None, 0) == GMX_EINVAL

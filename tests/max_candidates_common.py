"""The limit on a selection's candidates (gmx_engine_set_max_candidates): the cases and the expectation shared by
test_max_candidates.py (GPU) and test_max_candidates_host.py. The expectation comes from the oracle alone, task by task: its
search, its class map, and — for every task the limit does not leave out — its own quasimap_read."""
import functools

import numpy as np

from common import canonical_oracle
from oracle import Oracle
from oracle.oracle import RNG_LEMIRE
from gramtools_amd import master_seeds
from gramtools_amd.synth import bracket_to_ints, simulate_graph_reads
import test_read_outcomes
import test_read_positions
from test_read_outcomes import revcomp
from test_read_positions import half_sited_case

COV_KEYS = ("allele_sum", "grouped", "per_base", "allele_base", "depth")  # every key of common.canonical_* except stats


def ladder_case():
    """Flat, k = 6, 1 708 symbols: 120 random bases, then for 1, 2, 3, 5 and 8 copies a tandem block of that many copies of a fresh
    random 48-base unit followed by 120 random bases. Every copy carries its own two-allele SNP site at base 24 (built like
    test_many_instances.tandem_prg, the marker numbers running on across the blocks). 200 reads of 30 bases from each of two
    random haplotypes, every second one reverse-complemented: a read over the site of a block of c copies has c classes."""
    rng = np.random.default_rng(21)
    prg = [int(x) for x in rng.integers(1, 5, size=120)]
    m = 5
    for copies in (1, 2, 3, 5, 8):
        unit = rng.integers(1, 5, size=48, dtype=np.uint8)
        alt = int(unit[24]) % 4 + 1
        for _ in range(copies):
            prg += [int(x) for x in unit[:24]] + [m, int(unit[24]), m + 1, alt, m + 1] + [int(x) for x in unit[25:]]
            m += 2
        prg += [int(x) for x in rng.integers(1, 5, size=120)]
    reads = []
    for _ in range(2):
        hap, i = [], 0
        while i < len(prg):
            if prg[i] > 4:  # a site: [m, ref, m + 1, alt, m + 1]
                hap.append(prg[i + 1] if rng.random() < 0.5 else prg[i + 3])
                i += 5
            else:
                hap.append(prg[i])
                i += 1
        hap = np.asarray(hap, dtype=np.uint8)
        for j in range(200):
            st = int(rng.integers(0, hap.size - 30 + 1))
            r = hap[st:st + 30].copy()
            reads.append(revcomp(r) if j % 2 else r)
    return np.asarray(prg, dtype=np.uint32), 6, reads


def nested_ladder_case():
    """Nested, k = 5, 928 symbols, 22 sites: 80 random bases, then for 1, 2, 3 and 5 copies that many copies of a unit with a
    two-allele site whose second allele holds a SNP site, followed by 80 random bases. 400 reads of 24 bases from random walks."""
    rng = np.random.default_rng(33)

    def seq(n):
        return "".join("acgt"[int(x)] for x in rng.integers(0, 4, size=n))

    text = seq(80)
    for copies in (1, 2, 3, 5):
        a, b, c, d, e = seq(14), seq(5), seq(4), seq(3), seq(14)
        x = int(rng.integers(0, 4))  # a random base and the next one in acgt
        unit = a + "[" + b + "," + c + "[" + "acgt"[x] + "," + "acgt"[(x + 1) % 4] + "]" + d + "]" + e
        text += unit * copies + seq(80)
    prg = bracket_to_ints(text)
    return prg, 5, [np.asarray(r, dtype=np.uint8) for r in simulate_graph_reads(prg, 400, 24, 2)]


CASES = {"ladder": ladder_case, "nested_ladder": nested_ladder_case, "half_sited": half_sited_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """(prg, k, reads, seeds) of a named case."""
    prg, k, reads = CASES[name]()
    seeds = np.arange(1, len(reads) + 1, dtype=np.uint32) if name == "half_sited" else master_seeds(7, [len(reads)])
    return prg, k, reads, seeds


def describe_tasks(prg, k, reads, seeds, mode=RNG_LEMIRE):
    """Per task (2 i: read i as given, 2 i + 1: its reverse complement): (the oriented read, its seed, the outcome code and multi
    bit of test_read_outcomes.oracle_task, and pos, n, what of test_read_positions.oracle_task)."""
    o = Oracle(prg, k, rng_mode=mode)
    sa = o.sa()
    out = []
    for i, r in enumerate(reads):
        r = np.asarray(r, dtype=np.uint8)
        for x in (r, Oracle.reverse_complement(r) if r.size else r):
            code, multi = test_read_outcomes.oracle_task(o, k, x)
            pos, n, what = test_read_positions.oracle_task(o, sa, k, x, seeds[i], mode)
            out.append((x, int(seeds[i]), code, multi, pos, n, what))
    o.close()
    return out


def total_of(what):
    """The range of a task's draw, or 0 when it has no class (no draw, never left out)."""
    return what["nonvar"] + what["classes"] if what and what["classes"] else 0


def expect_from(prg, k, described, limit, mode=RNG_LEMIRE):
    """The expectation under `limit` (0: none) from describe_tasks' list: dict(cov: the oracle's canonical coverage without stats,
    bytes, positions, left_out: the task indices left out)."""
    o = Oracle(prg, k, rng_mode=mode)
    n_reads = len(described) // 2
    out = np.zeros(n_reads, dtype=np.uint8)
    positions = np.zeros((n_reads, 4), dtype=np.uint32)
    left_out = []
    for t, (x, seed, code, multi, pos, n, what) in enumerate(described):
        total = total_of(what)
        left = bool(limit) and total > limit
        if left:
            left_out.append(t)
            pos = min(what["positions"])  # nothing drawn: all its instances
        elif what is not None:
            o.quasimap_read(x, seed)
        assert multi == int(total > 1)
        out[t >> 1] |= code << (2 * (t & 1)) | (0 if left else multi) << (4 + (t & 1)) | int(left) << (6 + (t & 1))
        positions[t >> 1, 2 * (t & 1):2 * (t & 1) + 2] = (pos, n)
    cov = canonical_oracle(o)
    o.close()
    return dict(cov={key: cov[key] for key in COV_KEYS}, bytes=out, positions=positions, left_out=left_out)


@functools.lru_cache(maxsize=None)
def described(name):
    prg, k, reads, seeds = case(name)
    return describe_tasks(prg, k, reads, seeds)


@functools.lru_cache(maxsize=None)
def expectation(name, limit):
    prg, k, _, _ = case(name)
    return expect_from(prg, k, described(name), limit)


def allele_sum_total(cov):
    return sum(sum(site) for site in cov["allele_sum"])


def without_stats(canonical):
    return {key: canonical[key] for key in COV_KEYS}

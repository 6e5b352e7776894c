"""Links between nearby sites (gmx_engine_record_links): the case and the expectation shared by test_site_links.py
(GPU) and test_site_links_host.py. The expectation comes from the oracle alone: for each oriented read search_read_backwards;
the read is kept when the widths of its states sum to 1; locus_finder(state) gives its loci (its path plus the allele it starts
inside); the pairs are added in Python integers. The layout is the formula of include/gmx.h, computed here in numpy."""
import functools

import numpy as np

from oracle import Oracle

MAX_ALLELES = 8  # a site with more alleles is not linkable (the dense-counter limit)


# ---- the layout ------------------------------------------------------------------------------------------------------
def linkable(n_alleles):
    a = np.asarray(n_alleles, dtype=np.int64)
    return np.where(a <= MAX_ALLELES, a, 0)


def layout(n_alleles, span):
    """off[0 .. n_sites]: off[s + 1] - off[s] = A'(s) * sum_{d = 1..span} A'(s + d), A' = 0 past the last site."""
    a = linkable(n_alleles)
    n = a.size
    padded = np.concatenate([a, np.zeros(span + 1, dtype=np.int64)])
    right = np.zeros(n, dtype=np.int64)
    for d in range(1, span + 1):
        right += padded[d:d + n]
    return np.concatenate([[0], np.cumsum(a * right)]).astype(np.uint64)


def matrix_start(n_alleles, off, s, d):
    a = linkable(n_alleles)
    return int(off[s]) + int(a[s]) * int(sum(int(a[s + e]) for e in range(1, d) if s + e < a.size))


def block_of(n_alleles, span, matrices):
    """The link block of {(s, d): 2-D array} as one uint32 array."""
    off = layout(n_alleles, span)
    a = linkable(n_alleles)
    words = np.zeros(int(off[-1]), dtype=np.uint32)
    for (s, d), m in matrices.items():
        if d > span:
            continue
        assert m.shape == (a[s], a[s + d]) and m.size
        at = matrix_start(n_alleles, off, s, d)
        words[at:at + m.size] = m.reshape(-1)
    return off, words


# ---- the case --------------------------------------------------------------------------------------------------------
def links_case(seed=11, wide=True):
    """Flat, k = 5, about 1.5 kb of random reference with a site every 8-20 bases: 2-4-allele SNPs, indels (an empty allele and a
    3-6-base allele), ONE 10-allele site in the middle (not linkable; its grouped counts go through the log) and one stretch of
    about 120 bases, sites included, that stands a second time further on (a read inside it has two mapping instances). 700 reads
    of 40-80 bases from six random haplotypes, every second one reverse-complemented; the last 60 start inside a multi-base allele.
    wide=False: the same case with the first four alleles of that site only — no site uses the log, so an engine has its second
    workspace. Returns (prg, k, reads)."""
    rng = np.random.default_rng(seed)
    elems = []  # a base (int) or a site (list of alleles, each a list of bases)

    def site():
        u = rng.random()
        if u < 0.6:
            n = int(rng.integers(2, 5))
            return [[int(b)] for b in rng.permutation(4)[:n] + 1]
        if u < 0.8:
            return [[], [int(x) for x in rng.integers(1, 5, size=int(rng.integers(3, 7)))]]
        first = [int(x) for x in rng.integers(1, 5, size=int(rng.integers(3, 7)))]
        second = list(first)
        second[1] = second[1] % 4 + 1
        return [first, second, []][:int(rng.integers(2, 4))]

    def stretch(n_bases):
        out, n = [], 0
        while n < n_bases:
            gap = int(rng.integers(8, 21))
            out += [int(x) for x in rng.integers(1, 5, size=gap)]
            out.append(site())
            n += gap + 1
        return out

    elems += stretch(300)
    dup = stretch(120)
    elems += dup + stretch(330)
    wide_set = set()
    while len(wide_set) < 10:
        wide_set.add(tuple(int(x) for x in rng.integers(1, 5, size=3)))
    elems += [int(x) for x in rng.integers(1, 5, size=12)] + [[list(a) for a in sorted(wide_set)][:10 if wide else 4]]
    elems += stretch(300)
    elems += [int(x) for x in rng.integers(1, 5, size=10)] + [([list(a) for a in e] if isinstance(e, list) else e) for e in dup]
    elems += stretch(250) + [int(x) for x in rng.integers(1, 5, size=15)]
    prg, m = [], 5
    for e in elems:
        if isinstance(e, list):
            prg.append(m)
            for a in e:
                prg += a + [m + 1]
            m += 2
        else:
            prg.append(e)
    haps = []
    for _ in range(6):
        seq, inside = [], []  # inside: positions of the haplotype that lie inside a multi-base allele, its first base aside
        for e in elems:
            if isinstance(e, list):
                a = e[int(rng.integers(0, len(e)))]
                inside += list(range(len(seq) + 1, len(seq) + len(a)))
                seq += a
            else:
                seq.append(e)
        haps.append((np.asarray(seq, dtype=np.uint8), inside))
    reads = []
    for i in range(700):
        h, inside = haps[int(rng.integers(0, len(haps)))]
        n = int(rng.integers(40, 81))
        if i >= 640:
            st = int(inside[int(rng.integers(0, len(inside)))])
            st = min(st, h.size - n)
        else:
            st = int(rng.integers(0, h.size - n + 1))
        r = h[st:st + n].copy()
        reads.append((5 - r[::-1]).astype(np.uint8) if i % 2 else r)
    return np.asarray(prg, dtype=np.uint32), 5, reads


@functools.lru_cache(maxsize=None)
def case(wide=True):
    prg, k, reads = links_case(wide=wide)
    from gramtools_amd import master_seeds
    return prg, k, reads, master_seeds(7, [len(reads)])


# ---- the expectation -------------------------------------------------------------------------------------------------
def describe(prg, k, reads):
    """Per task (2 i: read i as given, 2 i + 1: its reverse complement): (the oriented read, n — the widths of its states summed —,
    the loci of its first state ascending by site as (site index, 0-based allele), whether the first of them is the allele the read
    starts inside)."""
    o = Oracle(prg, k)
    out = []
    for r in reads:
        r = np.asarray(r, dtype=np.uint8)
        for x in (r, Oracle.reverse_complement(r)):
            states = o.search_read_backwards(x)
            n = sum(hi - lo + 1 for lo, hi, _, _ in states)
            loci, starts_inside = [], False
            if states:
                _, found = o.locus_finder(states[0])
                loci = sorted(((marker - 5) >> 1, allele) for marker, allele in found)  # (the ids are the columns: pin_allele_order)
                inside_sites = {(marker - 5) >> 1 for marker, _ in states[0][3]}
                starts_inside = bool(loci) and loci[0][0] in inside_sites
            out.append((x, n, loci, starts_inside))
    o.close()
    return out


def pin_allele_order(prg, k, tasks, seeds):
    """The loci of the single-instance tasks, added as allele_sum[site][allele] += 1, are the allele-sum coverage of an oracle
    that maps exactly those tasks: locus_finder's allele ids are the columns of allele_sum_coverage as they stand."""
    o = Oracle(prg, k)
    mine = [[0] * len(site) for site in o.allele_sum()]
    for t, (x, n, loci, _) in enumerate(tasks):
        if n == 1:
            o.quasimap_read(x, int(seeds[t >> 1]))
            for s, a in loci:
                mine[s][a] += 1
    got = [list(site) for site in o.allele_sum()]
    o.close()
    assert got == mine and sum(sum(site) for site in mine) > 0


def matrices_of(n_alleles, tasks, span):
    """{(s, d): matrix} of every pair of linkable sites at most `span` apart (zero matrices included)."""
    a = linkable(n_alleles)
    out = {}
    for s in range(a.size):
        for d in range(1, span + 1):
            if a[s] and s + d < a.size and a[s + d]:
                out[(s, d)] = np.zeros((a[s], a[s + d]), dtype=np.uint32)
    for _, n, loci, _ in tasks:
        if n != 1:
            continue
        for i in range(len(loci)):
            for j in range(i + 1, len(loci)):
                (s, x), (t, y) = loci[i], loci[j]
                if 1 <= t - s <= span and (s, t - s) in out and x < a[s] and y < a[t]:
                    out[(s, t - s)][x, y] += 1
    return out


@functools.lru_cache(maxsize=None)
def described(wide=True):
    prg, k, reads, _ = case(wide)
    return describe(prg, k, reads)


@functools.lru_cache(maxsize=None)
def oracle_alleles(wide=True):
    prg, k, _, _ = case(wide)
    o = Oracle(prg, k)
    n = np.asarray([len(site) for site in o.allele_sum()], dtype=np.int64)
    o.close()
    return n


@functools.lru_cache(maxsize=None)
def expectation(span, wide=True):
    """(off, words) of the case's link block at `span`."""
    return block_of(oracle_alleles(wide), span, matrices_of(oracle_alleles(wide), described(wide), span))


def check_case_contents():
    """What the case must contain for the tests to mean anything, from the oracle's own description of it."""
    prg, k, reads, seeds = case()
    tasks, a = described(), linkable(oracle_alleles())
    pin_allele_order(prg, k, tasks, seeds)
    wide = [s for s in range(a.size) if a[s] == 0]
    assert len(wide) == 1 and 9 <= oracle_alleles()[wide[0]] <= 12
    m = matrices_of(oracle_alleles(), tasks, 3)
    for d in (1, 2, 3):
        assert any(mat.any() for (s, dd), mat in m.items() if dd == d), d
    # a pair whose left locus is the allele the read starts inside
    assert any(n == 1 and inside and len(loci) >= 2 and a[loci[0][0]] and a[loci[1][0]] and loci[1][0] - loci[0][0] <= 3
               for _, n, loci, inside in tasks)
    # a task with a pair skipped across (or at) the wide site whose other pairs count
    def skipped_and_counted(loci):
        sites = [s for s, _ in loci]
        return wide[0] in sites and sum(1 for s in sites if a[s]) >= 2 and any(
            a[s] and a[t] and 1 <= t - s <= 3 for i, s in enumerate(sites) for t in sites[i + 1:])
    assert any(n == 1 and skipped_and_counted(loci) for _, n, loci, _ in tasks)
    # tasks left out for n > 1 that cross two sites or more
    assert sum(1 for _, n, loci, _ in tasks if n > 1 and len(loci) >= 2) >= 5
    # a matrix with more than one non-zero cell in one row
    assert any((np.count_nonzero(mat, axis=1) > 1).any() for mat in m.values())
    return tasks

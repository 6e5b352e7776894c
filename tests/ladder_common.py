"""The coverage ladder's input families (tests/test_cover_ladder_host.py, tests/test_cover_ladder.py).

Which coverage instance records a task carries no semantics: a task that exceeds a scratch capacity — items, key sites (the
level-0 sites of an item's key), loci ((site, allele) pairs of an item, then of the drawn class), hull entries — has recorded
nothing and is handed to the next tier. Each family below is a small PRG with dials that move ONE of those numbers, and one
boundary read whose task sits on a capacity or one above it. The numbers themselves are read from the oracle (shape()), and
the expected coverage, read counters, outcome bytes and position records come from the oracle task by task
(max_candidates_common.describe_tasks / expect_from).

  A  enc(T)               T copies of a two-allele site whose first allele is 30 bases; the read lies inside that allele: ONE
                          pathless final state of T occurrences -> T items, T classes, one key site and one locus each. Up to
                          T = 5 the fast pass keeps it; 6 .. 64 go to the instance lanes, more to the large-capacity search.
  B  sited_plus_plain(S)  a unit with S SNP sites (one every 4 bases) and the same unit once more without sites; the read spans
                          the unit: 2 final states, 1 non-variant instance, 1 item with S key sites and S loci.
  C  tandem(T, S)         T copies of a unit, each with its own S sites: T states, T items, T classes, S key sites each.
                          T > 8 states or T * S > 48 path nodes leaves the fast pass for the large-capacity search.
  D  chains(depths, ...)  one unit whose level-0 sites are chains nested depths[i] deep (the read runs through the innermost
                          allele): one item, len(depths) key sites, sum(depths) loci. `pad` adds a base behind every inner
                          site, so a chain of depth d brings 2 d - 1 hull entries instead of d. `plain` appends the unit
                          without sites (a second final state: not a single-instance task); `copies` repeats the sited unit
                          (each copy an item and a class of its own, copies * sum(depths) path nodes).
  E  members(totals)      ONE level-0 site whose alleles each hold a copy of a chain unit with its own inner sites: the read
                          maps once per allele, every item has the same one-site key, so all are ONE class whose union has
                          sum(t + 1 for t in totals) loci.

Every batch is 32 reads over a 3-copy tandem block and their reverse complements (64 mapped tasks of 3 classes each, which
every run sends through the same instances) followed by the boundary read and its reverse complement, `repeat` times.
Neighbouring lanes of the same launch hold live scratch, so an overrun shows in someone's counts."""
import functools

import numpy as np

import max_candidates_common as mcc
from common import flatten_reads, _load_emu
from gramtools_amd.synth import bracket_to_ints
from oracle import Oracle

LETTERS = "acgt"
CAP_NAMES = ("lds", "mid", "regular", "big", "coop_item", "coop_class", "coop5_item", "coop5_class")
N_FILLER = 32  # reads over the 3-copy block; with their reverse complements 64 mapped multi-mapped tasks


@functools.lru_cache(maxsize=None)
def capacities():
    """The tiers' capacities as gmx_cover.h states them (through the host emulation's build of that header):
    {tier: dict(items, key_sites, loci, hull, path)} plus coop_units, single_loci, wide_loci."""
    import ctypes as C
    lib = _load_emu()
    out = (C.c_uint32 * 43)()
    lib.hostemu_capacities(out)
    caps = {name: dict(zip(("items", "key_sites", "loci", "hull", "path"), (int(x) for x in out[5 * t:5 * t + 5])))
            for t, name in enumerate(CAP_NAMES)}
    caps.update(coop_units=int(out[40]), single_loci=int(out[41]), wide_loci=int(out[42]))
    return caps


def _seq(rng, n):
    return "".join(LETTERS[int(x)] for x in rng.integers(0, 4, size=n))


def _other(ch, step=1):
    return LETTERS[(LETTERS.index(ch) + step) % 4]


def _num(text):
    return np.asarray([LETTERS.index(c) + 1 for c in text], dtype=np.uint8)


def revcomp(r):
    return (5 - np.asarray(r, dtype=np.uint8))[::-1].copy()


def _filler(rng):
    """(text, reads): a tandem block of 3 copies of a 48-base unit, each copy with its own SNP site at base 24, between random
    flanks; 32 reads of 30 bases over the site from the all-reference haplotype (3 states, 3 classes each)."""
    unit = _seq(rng, 48)
    site = "[" + unit[24] + "," + _other(unit[24]) + "]"
    text = _seq(rng, 40) + (unit[:24] + site + unit[25:]) * 3 + _seq(rng, 40)
    reads = []
    for j in range(N_FILLER):
        st = int(rng.integers(0, 18))  # the read covers base 24 of the unit it starts in
        reads.append(_num(unit[st:st + 30]))
    return text, reads


class Case:
    """One PRG and its batch: `reads` = the fillers, their reverse complements, then `repeat` times (boundary read, its reverse
    complement). A read r as given and revcomp(r)'s reverse-complement task are the same oriented read: every boundary read
    brings 2 mapped tasks."""

    def __init__(self, name, text, k, read, seed, repeat=1, extra=()):
        rng = np.random.default_rng(seed + 7000)
        filler_text, fillers = _filler(rng)
        self.name, self.k, self.repeat = name, k, repeat
        self.text = text + filler_text
        self.prg = bracket_to_ints(self.text)
        self.boundary = _num(read)
        self.filler_reads = [x for r in fillers for x in (r, revcomp(r))]
        self.reads = self.filler_reads + [self.boundary, revcomp(self.boundary)] * repeat
        self.reads += [x for r in extra for x in (_num(r), revcomp(_num(r)))]  # (further reads of the case's own, not boundary tasks)
        self.seeds = np.arange(1, len(self.reads) + 1, dtype=np.uint32) * np.uint32(2654435761)
        self.n_boundary_tasks = 2 * repeat

    def batch(self, with_boundary=True):
        reads = self.reads if with_boundary else self.filler_reads
        flat, offs = flatten_reads(reads)
        return flat, offs, self.seeds[:len(reads)]

    @functools.cached_property
    def described(self):
        return mcc.describe_tasks(self.prg, self.k, self.reads, self.seeds)

    @functools.lru_cache(maxsize=None)
    def expectation(self, limit=0):
        return mcc.expect_from(self.prg, self.k, self.described, limit)

    @functools.cached_property
    def want_stats(self):
        """The oracle's read counters of the batch (expect_from leaves them out)."""
        o = Oracle(self.prg, self.k)
        flat, offs, seeds = self.batch()
        o.map_reads(flat, offs, seeds)
        st = o.stats()
        o.close()
        return st

    @functools.cached_property
    def shape(self):
        """The boundary task as the oracle sees it: final states, units (one per path-bearing state, one per occurrence of a
        pathless one), path nodes, non-variant instances, items, classes, and the largest key, item loci set and class union."""
        o = Oracle(self.prg, self.k)
        states = o.search_read_backwards(self.boundary)
        enc = o.encapsulated(states)
        nonvar, entries = o.unique_site_paths(states)
        items = [st for st in enc if st[2] or st[3]]
        item_loci = [len(o.locus_finder(st)[1]) for st in items]
        hull = 0  # per class: the per-base nodes (DummyCovNode hull) of its members
        for _, members_of, _ in entries:
            of = [st for st in enc if (st[0], st[1]) in members_of and (st[2] or st[3])]
            hull = max(hull, len(o.dummy_cov_nodes(of, len(self.boundary))))
        out = dict(states=len(states), units=sum(1 if (tvd or tvg) else hi - lo + 1 for lo, hi, tvd, tvg in states),
                   path_nodes=sum(len(tvd) + len(tvg) for _, _, tvd, tvg in states), nonvar=nonvar, items=len(items),
                   classes=len(entries), key_sites=max((len(e[0]) for e in entries), default=0), item_loci=max(item_loci, default=0),
                   class_loci=max((len(e[2]) for e in entries), default=0), hull=hull,
                   single=len(states) == 1 and states[0][0] == states[0][1])
        o.close()
        return out


# ---- the families ------------------------------------------------------------------------------------------------------
def _flanked(rng, body):
    return _seq(rng, 40) + body + _seq(rng, 40)


@functools.lru_cache(maxsize=None)
def enc(T, repeat=1):
    rng = np.random.default_rng(100)
    allele = _seq(rng, 30)
    body = "".join("[" + allele + "," + _other(allele[0]) + "]" + _seq(rng, 6) for _ in range(T))
    return Case("enc(%d)" % T, _flanked(rng, body), 5, allele[5:25], 100 + T, repeat)


def _snp_unit(rng, S, min_len=0):
    """(bases, sited text): a unit of max(4 S + 3, min_len) bases with a SNP site at bases 2, 6, 10, ..."""
    bases = _seq(rng, max(4 * S + 3, min_len))
    sited = "".join("[" + c + "," + _other(c) + "]" if i % 4 == 2 and i // 4 < S else c for i, c in enumerate(bases))
    return bases, sited


@functools.lru_cache(maxsize=None)
def sited_plus_plain(S, repeat=1):
    rng = np.random.default_rng(200)
    bases, sited = _snp_unit(rng, S)
    return Case("sited_plus_plain(%d)" % S, _flanked(rng, sited + _seq(rng, 12) + bases), 5, bases, 200 + S, repeat)


@functools.lru_cache(maxsize=None)
def tandem(T, S, repeat=1, dead=False, tail=0):
    """dead: one more read, the boundary read with another first base — the search holds T states until its last step and ends
    without a final state. tail: site-free bases behind the last site (at least 4: the read's last 5-mer, the seed, is path-less
    and T positions wide; 0 and a unit of 4 S + 3 >= 30 bases: the seed spans the last site, T path-bearing states)."""
    rng = np.random.default_rng(300)
    bases, sited = _snp_unit(rng, S, max(30, 4 * S + 3 + tail))
    extra = (_other(bases[0]) + bases[1:],) if dead else ()
    return Case("tandem(%d,%d%s)" % (T, S, ",tail" if tail else ""), _flanked(rng, sited * T), 5, bases, 300 + 64 * T + S, repeat, extra)


def _chain(rng, d, pad):
    """(read bases, text) of a site nested d deep: [x [x [a,c] y, z] y, z] — the read runs through every first allele."""
    a = LETTERS[int(rng.integers(0, 4))]
    read, text = a, "[" + a + "," + _other(a) + "]"
    for _ in range(d - 1):
        x, y = LETTERS[int(rng.integers(0, 4))], (LETTERS[int(rng.integers(0, 4))] if pad else "")
        read, text = x + read + y, "[" + x + text + y + "," + _other(x, 2) + "]"
    return read, text


def _chain_unit(rng, depths, pad, gap=3):
    read, text = _seq(rng, 6), ""
    text = read
    for d in depths:
        r, t = _chain(rng, d, pad)
        g = _seq(rng, gap)
        read, text = read + r + g, text + t + g
    tail = _seq(rng, 6)
    return read + tail, text + tail


@functools.lru_cache(maxsize=None)
def chains(depths, plain=False, pad=False, copies=1, repeat=1):
    rng = np.random.default_rng(400)
    read, text = _chain_unit(rng, depths, pad)
    body = text
    for _ in range(copies - 1):  # (each copy with site markers of its own, the same bases)
        body += text
    if plain:
        body += _seq(rng, 12) + read
    name = "chains(%s%s%s%s)" % ("+".join(map(str, depths)), ",plain" if plain else "", ",pad" if pad else "", ",x%d" % copies if copies > 1 else "")
    return Case(name, _flanked(rng, body), 5, read, 400 + sum(depths) + 100 * len(depths), repeat)


@functools.lru_cache(maxsize=None)
def members(totals, repeat=1):
    """`totals`: per allele of the enclosing site, the depths of its copy's chains as a tuple (depth 0: no site, the bare base)."""
    rng = np.random.default_rng(500)
    n = len(totals[0])
    bases = [(LETTERS[int(rng.integers(0, 4))], LETTERS[int(rng.integers(0, 4))], _seq(rng, 3)) for _ in range(n)]
    head, tail = _seq(rng, 6), _seq(rng, 6)
    read = head + "".join(x + a + g for x, a, g in bases) + tail
    alleles = []
    for depths in totals:
        t = head
        for (x, a, g), d in zip(bases, depths):
            if d == 0:
                t += x + a + g
            elif d == 1:
                t += x + "[" + a + "," + _other(a) + "]" + g
            else:
                t += "[" + x + "[" + a + "," + _other(a) + "]" + "," + _other(x, 2) + "]" + g
        alleles.append(t + tail)
    text = _flanked(rng, "[" + ",".join(alleles) + "]")
    name = "members(%s)" % "|".join(str(sum(d)) for d in totals)
    return Case(name, text, 5, read, 500 + sum(sum(d) for d in totals), repeat)


def _deep(rng, d, inner):
    """`inner` as the first allele of a site nested d deep (d = 0: bare): [x [x [inner,c], z], z]."""
    text = inner
    for _ in range(d):
        x = LETTERS[int(rng.integers(0, 4))] if text is not inner else ""
        text = "[" + x + text + "," + _other(inner[0], 2) + "]"
    return text


@functools.lru_cache(maxsize=None)
def deep(depths, plain=False, repeat=1, separate=False):
    """D without path nodes: one level-0 site whose alleles each hold a 30-base sequence nested depths[i] deep (the level-0 site
    included); the 20-base read lies inside that sequence: ONE pathless state of len(depths) occurrences, one encapsulated item
    each with depths[i] loci (its site and all its parents), one key site, ONE class whose union has sum(depths) loci and
    len(depths) hull entries. `plain`: the bare sequence once more outside (a non-variant instance). `separate`: every chain a
    level-0 site of its own instead — len(depths) classes of one item each."""
    rng = np.random.default_rng(600)
    inner = _seq(rng, 30)
    if separate:
        body = "".join(_deep(rng, d, inner) + _seq(rng, 6) for d in depths)
    elif len(depths) == 1:
        body = _deep(rng, depths[0], inner)
    else:
        body = "[" + ",".join(_deep(rng, d - 1, inner) for d in depths) + "]"
    if plain:
        body += _seq(rng, 12) + inner
    name = "deep(%s%s%s)" % ("+".join(map(str, depths)), ",plain" if plain else "", ",separate" if separate else "")
    return Case(name, _flanked(rng, body), 5, inner[5:25], 600 + sum(depths) + 1000 * len(depths), repeat)


# ---- the ladder, as a statement over the oracle's numbers ------------------------------------------------------------------
ROUTE_KEYS = ("general", "general_rest", "coop_rejected_general", "coop_rejected_inst", "coop_rejected_big", "mid", "overflow", "huge_cover",
              "huge_search", "big_mapped", "inst_mapped")


def exceeds(shape, caps, class_drawn=True):
    """Whether a task of this shape exceeds a one-lane tier of these capacities (gmx_cover_task's checks in their order: items,
    then every item's loci and key, then — when the draw falls on a class — that class's union and hull). The largest class
    stands for the drawn one: on the families here all classes of a task are alike."""
    if shape["items"] > caps["items"] or shape["item_loci"] > caps["loci"] or shape["key_sites"] > caps["key_sites"]:
        return True
    return class_drawn and (shape["class_loci"] > caps["loci"] or shape["hull"] > caps["hull"])


def coop_rejects(shape, caps, class_drawn=True, five=False):
    """The cooperative instances' reject rule: more than 16 units, an item beyond an item lane's scratch, or the drawn class
    beyond the class scratch."""
    item, cls = caps["coop5_item" if five else "coop_item"], caps["coop5_class" if five else "coop_class"]
    if shape["units"] > caps["coop_units"] or shape["item_loci"] > item["loci"] or shape["key_sites"] > item["key_sites"]:
        return True
    return class_drawn and (shape["class_loci"] > cls["loci"] or shape["hull"] > cls["hull"])


def expected_route(shape, source, coop=True, one=True, class_drawn=True):
    """For ONE boundary task, how much longer each queue of Quasimapper.debug_cover_counts gets: the ladder of gmx_engine_batch.h
    over the oracle's numbers. `source`: which search finishes the task — "fast" (the fast pass's general queue), "inst" (a
    path-less seed over 6 .. 64 positions, GMX_SEED_SPLIT_MAX .. GMX_INST_MAX: one lane per instance, queue 5) or "big" (the
    large-capacity search, queue 2). It is the pair's own statement, proven by the inst_mapped / big_mapped counters."""
    caps = capacities()
    r = dict.fromkeys(ROUTE_KEYS, 0)
    if source == "fast":
        if shape["single"] and shape["item_loci"] <= caps["single_loci"]:
            return r  # a compact record: gmx_cover_single_kernel records it (these PRGs are nested)
        r["general"] = 1
        if one and shape["single"] and shape["item_loci"] <= caps["wide_loci"]:
            return r  # gmx_cover_one_kernel records it
        r["general_rest"] = 1
        if coop:
            if not coop_rejects(shape, caps, class_drawn):
                return r
            r["coop_rejected_general"] = 1
        if not exceeds(shape, caps["lds"], class_drawn):
            return r
        r["mid"] = 1
        if not exceeds(shape, caps["regular"], class_drawn):
            return r
    else:
        r["inst_mapped" if source == "inst" else "big_mapped"] = 1
        if coop:
            if not coop_rejects(shape, caps, class_drawn, five=source == "inst"):
                return r
            r["coop_rejected_inst" if source == "inst" else "coop_rejected_big"] = 1
        if not exceeds(shape, caps["mid"], class_drawn):
            return r
    r["overflow"] = 1
    if exceeds(shape, caps["big"], class_drawn):
        r["huge_cover"] = 1
    return r


def boundary_route(case, source, coop=True, one=True):
    """The sum of expected_route over the case's boundary tasks; whether a task's draw falls on a class is the oracle's
    (describe_tasks: r against the non-variant instances)."""
    total = dict.fromkeys(ROUTE_KEYS, 0)
    n = 0
    for t, (_, _, _, _, _, _, what) in enumerate(case.described):
        if t < 2 * len(case.filler_reads) or t >= 2 * (len(case.filler_reads) + case.n_boundary_tasks) or what is None:
            continue
        n += 1
        drawn = what["classes"] > 0 and what["r"] > what["nonvar"]
        for key, v in expected_route(case.shape, source, coop, one, drawn).items():
            total[key] += v
    assert n == case.n_boundary_tasks, (n, case.n_boundary_tasks)
    return total


class Pair:
    """One hand-over on one dimension: a case AT the capacity and one with ONE MORE. `tier`, `dim`: whose capacity (capacities());
    `key`: the oracle's number that sits on it (Case.shape); `watch`: the queue of debug_cover_counts that gets the task only
    in the second case; `source`: which search finishes the boundary task; `coop`: with the cooperative instances."""

    def __init__(self, name, tier, dim, key, watch, at, over, source="fast", coop=False):
        self.name, self.tier, self.dim, self.key, self.watch, self.at, self.over, self.source, self.coop = \
            name, tier, dim, key, watch, at, over, source, coop

    def capacity(self):
        caps = capacities()
        return caps[self.tier] if self.dim is None else caps[self.tier][self.dim]


def _p(*a, **kw):
    return Pair(*a, **kw)


X4, X2 = (4,), (2,)
PAIRS = [
    # the one-lane tiers of the fast pass's tasks (GMX_NO_COOP=1: nothing in front of them)
    _p("lds-items", "lds", "items", "items", "mid", lambda: enc(4), lambda: enc(5)),
    _p("lds-key-sites", "lds", "key_sites", "key_sites", "mid", lambda: sited_plus_plain(12), lambda: sited_plus_plain(13)),
    _p("lds-item-loci", "lds", "loci", "item_loci", "mid", lambda: deep((24,), plain=True), lambda: deep((25,), plain=True)),
    _p("lds-class-loci", "lds", "loci", "class_loci", "mid", lambda: deep((12, 12)), lambda: deep((12, 13))),
    _p("lds-hull", "lds", "hull", "hull", "mid", lambda: chains((4, 4, 4, 2), plain=True, pad=True), lambda: chains((5, 5, 4), plain=True, pad=True)),
    _p("regular-key-sites", "regular", "key_sites", "key_sites", "overflow", lambda: sited_plus_plain(16), lambda: sited_plus_plain(17)),
    _p("regular-item-loci", "regular", "loci", "item_loci", "overflow", lambda: deep((64,), plain=True), lambda: deep((65,), plain=True)),
    _p("regular-class-loci", "regular", "loci", "class_loci", "overflow", lambda: deep((32, 32)), lambda: deep((32, 33))),
    _p("big-items", "big", "items", "items", "huge_cover", lambda: enc(1024), lambda: enc(1025), source="big"),
    _p("big-key-sites", "big", "key_sites", "key_sites", "huge_cover", lambda: sited_plus_plain(32), lambda: sited_plus_plain(33)),
    # the one-lane tier of the instance-searched and the large-capacity tasks
    _p("mid-items", "mid", "items", "items", "overflow", lambda: tandem(12, 2), lambda: tandem(13, 2), source="inst"),
    _p("mid-key-sites", "mid", "key_sites", "key_sites", "overflow", lambda: tandem(5, 12), lambda: tandem(5, 13), source="big"),
    _p("mid-item-loci", "mid", "loci", "item_loci", "overflow", lambda: chains(X4 * 12, copies=2), lambda: chains(X4 * 11 + (5,), copies=2), source="big"),
    _p("mid-class-loci", "mid", "loci", "class_loci", "overflow", lambda: deep((8,) * 6), lambda: deep((8,) * 5 + (9,)), source="inst"),
    # the cooperative instances in front of them: 3 (the fast pass's tasks), 2 (large-capacity), 5 (instance-searched)
    _p("coop3-key-sites", "coop_item", "key_sites", "key_sites", "coop_rejected_general", lambda: sited_plus_plain(16), lambda: sited_plus_plain(17), coop=True),
    _p("coop3-item-loci", "coop_item", "loci", "item_loci", "coop_rejected_general", lambda: deep((24,), plain=True), lambda: deep((25,), plain=True), coop=True),
    _p("coop3-class-loci", "coop_class", "loci", "class_loci", "coop_rejected_general", lambda: deep((16, 16, 16)), lambda: deep((16, 16, 17)), coop=True),
    _p("coop2-units", "coop_units", None, "units", "coop_rejected_big", lambda: tandem(16, 7), lambda: tandem(17, 7), source="big", coop=True),
    _p("coop2-key-sites", "coop_item", "key_sites", "key_sites", "coop_rejected_big", lambda: tandem(5, 16), lambda: tandem(5, 17), source="big", coop=True),
    _p("coop2-item-loci", "coop_item", "loci", "item_loci", "coop_rejected_big", lambda: chains(X2 * 12, copies=2), lambda: chains(X2 * 11 + (3,), copies=2),
       source="big", coop=True),
    _p("coop5-units", "coop_units", None, "units", "coop_rejected_inst", lambda: enc(16), lambda: enc(17), source="inst", coop=True),
    _p("coop5-key-sites", "coop5_item", "key_sites", "key_sites", "coop_rejected_inst", lambda: tandem(9, 8, tail=5), lambda: tandem(9, 9, tail=5), source="inst", coop=True),
    _p("coop5-item-loci", "coop5_item", "loci", "item_loci", "coop_rejected_inst", lambda: deep((12,) * 6, separate=True), lambda: deep((12,) * 5 + (13,), separate=True),
       source="inst", coop=True),
    _p("coop5-class-loci", "coop5_class", "loci", "class_loci", "coop_rejected_inst", lambda: deep(X4 * 6), lambda: deep(X4 * 5 + (5,)), source="inst", coop=True),
    # single-instance tasks: the compact record's loci, then gmx_cover_one_kernel's
    _p("single-loci", "single_loci", None, "item_loci", "general", lambda: deep((8,)), lambda: deep((9,)), coop=True),
    _p("wide-loci", "wide_loci", None, "item_loci", "general_rest", lambda: deep((32,)), lambda: deep((33,)), coop=True),
]
PAIRS_BY_NAME = {p.name: p for p in PAIRS}


# ---- the host emulation over a case -----------------------------------------------------------------------------------------
def hostemu_run(case, with_boundary=True, fast_states=8, fast_arena=48, seed_split=5, **kw):  # (GMX_FAST_STATES, GMX_FAST_ARENA, GMX_SEED_SPLIT_MAX)
    """(canonical coverage, {hand-over: count}) of the host emulation at the engine's real capacities."""
    from common import hostemu_map
    reads = case.reads if with_boundary else case.filler_reads
    counts = {}
    cov, _, rc = hostemu_map(case.prg, case.k, reads, case.seeds[:len(reads)], fast_states=fast_states, fast_arena=fast_arena, coop=True, seed_split=seed_split,
                             counts=counts, **kw)
    assert rc == 0, rc
    return cov, counts

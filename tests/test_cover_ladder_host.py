"""The coverage ladder on the host: the input families of tests/ladder_common.py against the oracle, and the host
emulation — gmx_cover.h at the engine's real tier capacities, Lds -> CoverEnv -> Big -> Dyn for the fast pass's tasks and
Mid -> Big -> Dyn for the large-capacity search's — against the oracle and against the ladder as ladder_common states it.
Every pair sits ON a capacity and ONE above it; the numbers are the oracle's (Case.shape), the capacities gmx_cover.h's."""
import re

import pytest

import ladder_common as lc
from common import ROOT

NAMES = [p.name for p in lc.PAIRS]


def test_the_capacities_are_stated_once_and_the_engine_builds_its_tiers_from_them():
    caps = lc.capacities()
    assert caps["lds"] == dict(items=4, key_sites=12, loci=24, hull=24, path=8)
    assert caps["mid"] == dict(items=12, key_sites=12, loci=48, hull=48, path=8)
    assert caps["regular"] == dict(items=24, key_sites=16, loci=64, hull=64, path=8)
    assert caps["big"] == dict(items=1024, key_sites=32, loci=1024, hull=1024, path=8)
    assert caps["coop_item"] == dict(items=1, key_sites=16, loci=24, hull=1, path=24)
    assert caps["coop_class"] == dict(items=1, key_sites=1, loci=48, hull=48, path=8)
    assert caps["coop5_item"] == dict(items=1, key_sites=8, loci=12, hull=1, path=8)
    assert caps["coop5_class"] == dict(items=1, key_sites=1, loci=24, hull=24, path=8)
    assert (caps["coop_units"], caps["single_loci"], caps["wide_loci"]) == (16, 8, 32)
    kernels = open(ROOT + "/gramtools_amd/csrc/gmx_engine_cover_kernels.h").read()
    emu = open(ROOT + "/tests/hostemu/hostemu.cpp").read()
    for text in (kernels, emu):  # no tier states its capacities as numbers any more
        assert not re.search(r"(CoverEnvT|EmuEnvT)<\s*\d", text)
    for name in ("LDS", "MID", "REGULAR", "BIG", "COOP_ITEM", "COOP_CLASS", "COOP5_ITEM", "COOP5_CLASS"):
        assert "GMX_TIER_ARGS(GMX_CAPS_%s)" % name in kernels
    for name in ("LDS", "MID", "REGULAR", "BIG", "COOP_ITEM", "COOP5_ITEM"):
        assert "GMX_TIER_ARGS(GMX_CAPS_%s)" % name in emu


def test_the_cover_counts_hook_is_declared_guarded_and_bound():
    from gramtools_amd import Quasimapper, _lib
    header = open(ROOT + "/include/gmx.h").read()
    assert re.search(r"\bint\s+gmx_debug_cover_counts\(gmx_engine \*e, uint64_t out\[12\]\);", header)
    source = open(ROOT + "/gramtools_amd/csrc/gmx_engine_readback.h").read()
    assert re.search(r"int gmx_debug_cover_counts\([^)]*\) try \{.*?\} GMX_GUARD_INT\(\"gmx_debug_cover_counts\"\)", source, re.S)
    assert "gmx_debug_cover_counts" in _lib.SYMBOLS and hasattr(_lib.load(), "gmx_debug_cover_counts")
    assert callable(Quasimapper.debug_cover_counts) and len(Quasimapper.COVER_COUNTS) == 12


@pytest.mark.parametrize("name", NAMES)
def test_each_pair_sits_on_its_capacity_and_one_above(name):
    """The oracle's numbers of the two boundary tasks: the pair's dimension is the capacity and the capacity + 1, and no
    other dimension of that tier is exceeded — so the dimension is the one reason for the hand-over."""
    pair = lc.PAIRS_BY_NAME[name]
    cap, caps = pair.capacity(), lc.capacities()
    at, over = pair.at().shape, pair.over().shape
    print(name, cap, at, over)
    assert at[pair.key] == cap and over[pair.key] == cap + 1, (cap, at, over)
    reduced = dict(over, **{pair.key: cap})
    if pair.key == "item_loci":  # (an item's loci are its class's too, and a crossed site brings its per-base node)
        reduced.update(class_loci=at["class_loci"], hull=at["hull"])
    if pair.tier in ("lds", "mid", "regular", "big"):
        assert not lc.exceeds(at, caps[pair.tier])
        assert lc.exceeds(over, caps[pair.tier])
        assert not lc.exceeds(reduced, caps[pair.tier])
    elif pair.tier.startswith("coop"):
        five = pair.source == "inst"
        assert not lc.coop_rejects(at, caps, five=five) and lc.coop_rejects(over, caps, five=five)
        assert not lc.coop_rejects(reduced, caps, five=five)


@pytest.mark.parametrize("which", ["at", "over"])
@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith(("single", "wide"))])
def test_the_emulation_at_the_real_capacities_gives_the_oracles_coverage_and_the_stated_hand_overs(name, which):
    pair = lc.PAIRS_BY_NAME[name]
    case = getattr(pair, which)()
    want = case.expectation()
    cov, counts = lc.hostemu_run(case)
    _, base = lc.hostemu_run(case, with_boundary=False)
    assert {key: cov[key] for key in want["cov"]} == want["cov"]
    assert cov["stats"] == case.want_stats
    delta = {key: counts[key] - base[key] for key in counts}
    print(case.name, case.shape, delta)
    n = case.n_boundary_tasks
    serial, coop = lc.boundary_route(case, pair.source, coop=False), lc.boundary_route(case, pair.source, coop=True)
    # (the emulation has one search behind the fast pass: the instance lanes' tasks are among its large-capacity ones)
    assert delta["general_big"] == (n if pair.source != "fast" else 0) and delta["general_fast"] == (0 if pair.source != "fast" else n)
    assert delta["lds_to_regular"] == serial["mid"]
    assert delta["regular_to_big"] + delta["mid_to_big"] == delta["cover_overflow"] == serial["overflow"]
    assert delta["cover_huge"] == serial["huge_cover"]
    assert delta["coop_reject_fast"] == coop["coop_rejected_general"]
    assert delta["coop5_reject_big" if pair.source == "inst" else "coop_reject_big"] == coop["coop_rejected_inst"] + coop["coop_rejected_big"]
    # the pair's own hand-over: nothing at the capacity, every boundary task one above it
    watched = {"mid": delta["lds_to_regular"], "overflow": delta["cover_overflow"], "huge_cover": delta["cover_huge"],
               "coop_rejected_general": delta["coop_reject_fast"], "coop_rejected_big": delta["coop_reject_big"],
               "coop_rejected_inst": delta["coop5_reject_big"]}[pair.watch]
    if which == "at":
        assert watched == 0
    elif pair.key in ("class_loci", "hull") and case.shape["nonvar"]:
        assert watched == sum(1 for t, d in enumerate(case.described) if t >= 2 * len(case.filler_reads) and d[6] and d[6]["r"] > d[6]["nonvar"])
    else:
        assert watched == n


@pytest.mark.parametrize("which", ["at", "over"])
@pytest.mark.parametrize("name", ["single-loci", "wide-loci"])
def test_the_emulations_single_instance_routines_at_their_loci_capacities(name, which):
    """gmx_cover_single_nested (GMX_SINGLE_LOCI) and gmx_cover_single_nested_wide (GMX_WIDE_LOCI): a task with one locus more is
    left to the general routine, and either way the coverage is the oracle's."""
    pair = lc.PAIRS_BY_NAME[name]
    case = getattr(pair, which)()
    want = case.expectation()
    stats = {}
    cov, counts = lc.hostemu_run(case, wide=name == "wide-loci", stats=stats)
    base_stats = {}
    lc.hostemu_run(case, with_boundary=False, wide=name == "wide-loci", stats=base_stats)
    assert {key: cov[key] for key in want["cov"]} == want["cov"] and cov["stats"] == case.want_stats
    if name == "wide-loci":
        assert stats["n_wide"] - base_stats["n_wide"] == (case.n_boundary_tasks if which == "at" else 0), (stats, base_stats)


def test_the_families_the_gpu_suite_adds_give_the_oracles_coverage_on_the_host():
    """The cases of tests/test_cover_ladder.py that no pair holds (the emulation has no heap-backed search: tandem(1025, 2) is
    left to the GPU)."""
    for case in (lc.tandem(2, 13), lc.tandem(2, 33), lc.tandem(5, 17), lc.tandem(17, 4), lc.tandem(25, 3), lc.chains((4, 4)), lc.chains((4, 5)),
                 lc.chains((4, 4), plain=True), lc.members(((1,) * 11, (1,) * 11)), lc.sited_plus_plain(33, repeat=3)):
        want = case.expectation()
        cov, counts = lc.hostemu_run(case)
        assert {key: cov[key] for key in want["cov"]} == want["cov"], case.name
        assert cov["stats"] == case.want_stats, case.name

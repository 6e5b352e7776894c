"""The coverage ladder on the device. Which instance records a task carries no semantics — the compact records,
gmx_cover_one_kernel, the 16-lane cooperative kernels, the one-lane LDS instances (CoverEnvLds, CoverEnvMid, CoverEnv), the
global-memory CoverEnvBig, the heap-backed last tier — and every hand-over is a capacity check followed by a push to the next
queue. Each case puts ONE task on a capacity or one above it (tests/ladder_common.py: the numbers are the oracle's), among 64
ordinary multi-mapped tasks whose lanes hold live scratch in the same launches, and asserts

  * the oracle's coverage, read counters, outcome bytes and position records, and
  * the route, exactly, from Quasimapper.debug_cover_counts: every queue of the ladder is as much longer than in the same
    batch without the boundary tasks as ladder_common.expected_route says — nothing at the capacity, every boundary task
    one above it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ladder_common as lc
import site_ambiguity_common as sac
from common import canonical_cov
from gramtools_amd import Index, Quasimapper
from gramtools_amd._lib import GmxError
from oracle import Oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("GMX_NO_COOP", "GMX_NO_COVER_ONE", "GMX_NO_COVER_JUMP", "GMX_NO_INST")
GMX_EHIP = -3  # include/gmx.h
_index = {}


def index_of(case):
    if case.name not in _index:
        _index[case.name] = Index(case.prg, case.k)
    return _index[case.name]


class Run:
    """One engine, one launch of the case's batch (with or without its boundary tasks)."""

    def __init__(self, case, env=(), with_boundary=True, recordings=False, limit=0, **engine_kw):
        try:
            self._run(case, env, with_boundary, recordings, limit, engine_kw)
        except GmxError as exc:
            if exc.code != GMX_EHIP:  # (a wrong argument, GMX_ECAP, ...: this test's failure)
                raise
            # a HIP runtime error — a fault on the device among them — is no finding of a comparison: nothing more is started there
            pytest.exit("HIP error in %s %s: %r" % (case.name, env, exc), returncode=3)

    def _run(self, case, env, with_boundary, recordings, limit, engine_kw):
        with pytest.MonkeyPatch.context() as mp:
            for v in SWITCHES:
                mp.delenv(v, raising=False)
            for v in env:
                mp.setenv(v, "1")
            qm = Quasimapper(index_of(case), **engine_kw)
            qm.record_outcomes()
            qm.record_positions()
            if recordings:
                qm.record_strands()
                qm.record_site_ambiguity()
            if limit:
                qm.set_max_candidates(limit)
            flat, offs, seeds = case.batch(with_boundary)
            qm.map_reads(flat, offs, seeds)
            self.cov = canonical_cov(qm.coverage())
            self.counts = qm.debug_cover_counts()
            self.outcomes, self.positions = qm.outcomes(), qm.positions()
            if recordings:
                self.strands = [canonical_cov(qm.coverage(strand=s)) for s in (0, 1)]
                self.ambiguity = qm.site_ambiguity()
            qm.close()


def check_results(case, run, note, limit=0):
    want = case.expectation(limit)
    assert {key: run.cov[key] for key in want["cov"]} == want["cov"], note
    assert run.cov["stats"] == case.want_stats, note
    bad = np.flatnonzero(run.outcomes != want["bytes"])
    assert bad.size == 0, (note, [(int(i), int(run.outcomes[i]), int(want["bytes"][i])) for i in bad[:10]])
    bad = np.flatnonzero((run.positions != want["positions"]).any(axis=1))
    assert bad.size == 0, (note, [(int(i), run.positions[i].tolist(), want["positions"][i].tolist()) for i in bad[:10]])


def delta(run, base):
    return {key: run.counts[key] - base.counts[key] for key in lc.ROUTE_KEYS}


# ---- 3, 4: the boundaries, each route proven by the counters ---------------------------------------------------------------
@pytest.mark.parametrize("which", ["at", "over"])
@pytest.mark.parametrize("name", [p.name for p in lc.PAIRS])
def test_boundary(name, which):
    pair = lc.PAIRS_BY_NAME[name]
    case = getattr(pair, which)()
    env = () if pair.coop else ("GMX_NO_COOP",)
    run, base = Run(case, env), Run(case, env, with_boundary=False)
    got, want = delta(run, base), lc.boundary_route(case, pair.source, coop=pair.coop)
    print(case.name, env, case.shape, "\n  route", got, "\n  batch", run.counts)
    check_results(case, run, case.name)
    assert got == want, (case.name, got, want)
    if which == "at":
        assert got[pair.watch] == 0
    elif not (pair.key in ("class_loci", "hull") and case.shape["nonvar"]):  # (there only the tasks whose draw falls on the class)
        assert got[pair.watch] == case.n_boundary_tasks


def test_two_final_states_are_left_to_the_general_instances_whatever_their_loci():
    """gmx_cover_one_kernel takes tasks of ONE final state: sited_plus_plain(12) has 12 loci, well inside GMX_WIDE_LOCI, and two
    final states — both boundary tasks pass through its queue to general_rest, where the cooperative kernel records them."""
    case = lc.sited_plus_plain(12)
    run, base = Run(case), Run(case, with_boundary=False)
    got = delta(run, base)
    print(case.name, case.shape, got)
    check_results(case, run, case.name)
    assert case.shape["item_loci"] == 12 and case.shape["units"] == 2 and not case.shape["single"]
    assert got == lc.boundary_route(case, "fast") and got["general"] == got["general_rest"] == 2 and got["coop_rejected_general"] == 0


@pytest.mark.parametrize("T", [6, 24, 25])
def test_a_path_less_seed_over_six_positions_never_reaches_the_fast_pass_tiers(T):
    """Why CoverEnv's 24 items and the 16 units of cooperative instance 3 have no pair: enc(5) is recorded behind the fast
    pass (the lds-items pair), enc(6) already leaves at the seed kernel (GMX_SEED_SPLIT_MAX) for the instance lanes, and so do 24
    and 25 occurrences — queue 5, cooperative instance 5, CoverEnvMid; the general queue of the fast pass never sees them."""
    case = lc.enc(T)
    run, base = Run(case), Run(case, with_boundary=False)
    got = delta(run, base)
    print(case.name, case.shape, got)
    check_results(case, run, case.name)
    assert case.shape["items"] == case.shape["units"] == T
    assert got == lc.boundary_route(case, "inst") and got["inst_mapped"] == 2 and got["general"] == got["mid"] == 0
    assert got["coop_rejected_inst"] == got["overflow"] == (2 if T > 16 else 0)


# ---- 5: the last tier's second round -------------------------------------------------------------------------------------------
def tail_words(n_items, read_len, whole_heap_words=0):
    """gmx_tail_item's arithmetic: the scratch words a coverage item needs before its loci and hull (five words each, at least
    64 of them): n_items * (ITEM_W + 2 + cap_b) + 2 * GMX_PATH_CACHE + 1 + 5 * 64, cap_b = min(max(len + 8, 32), 4096) key sites
    per item. In the second round (whole_heap_words: lane 0 with all of the heap) the routine is generous with key sites:
    cap_b is at least min(65 536, heap words / (4 n_items))."""
    cap_b = min(max(read_len + 8, 32), 4096)
    if whole_heap_words:
        cap_b = max(cap_b, min(65536, whole_heap_words // (4 * n_items)))
    return n_items * (6 + 2 + cap_b) + 2 * 8 + 1 + 5 * 64


def test_a_cover_item_that_does_not_fit_its_slice_is_redone_with_the_whole_heap():
    """sited_plus_plain(33), three times: 6 tasks beyond CoverEnvBig's 32 key sites (huge_cover). One item, a 135-base read: 488
    words. A heap of 128 KiB gives every lane a slice of 512 words: no retry. 64 KiB gives 256: all six are redone by lane 0
    with the whole heap: 16 384 words, of which the second round's 4 096 key sites take 4 441 — the one item fits, unlike the
    6 000 instances of test_many_instances' GMX_ECAP case at the same heap. The result is the oracle's either way."""
    case = lc.sited_plus_plain(33, repeat=3)
    assert case.shape["items"] == 1 and len(case.boundary) == 135 and tail_words(1, 135) == 488
    for heap, retries in ((128 << 10, 0), (64 << 10, 6)):
        heap_words = heap // 4
        assert (heap_words // 64 >= 488) == (retries == 0)  # a lane's slice holds the item, or not
        assert tail_words(1, 135, heap_words) <= heap_words and (heap_words - tail_words(1, 135, heap_words)) // 5 >= 33  # the whole heap does, with 33 loci
        run, base = Run(case, huge_heap_bytes=heap), Run(case, with_boundary=False, huge_heap_bytes=heap)
        print(case.name, heap, run.counts)
        check_results(case, run, (case.name, heap))
        assert run.counts["huge_cover"] - base.counts["huge_cover"] == 6 and run.counts["huge_search"] == 0
        assert run.counts["tail_retry"] == retries and base.counts["tail_retry"] == 0


def test_a_search_item_that_does_not_fit_its_slice_is_redone_with_the_whole_heap():
    """tandem(1025, 2), twice: 4 tasks with 1 025 final states against the large-capacity slots' 1 024 (huge_search). The search
    pools take 30 words per state, half of the slice at most; 1 025 items of a 30-base read then need 1 025 * 46 + 337 = 47 487
    words of the other half. 32 MiB: slices of 131 072 words, no retry. 8 MiB: slices of 32 768 words hold the 1 025 states and not
    the scratch: all four are redone with the whole heap."""
    case = lc.tandem(1025, 2, repeat=2)
    assert tail_words(1025, 30) == 47487
    for heap, retries in ((32 << 20, 0), (8 << 20, 4)):
        slice_words = heap // 4 // 64
        assert slice_words // 30 >= 1025 and (slice_words - 15 * (slice_words // 30) >= 47487) == (retries == 0)
        run = Run(case, huge_heap_bytes=heap)
        print(case.name, heap, run.counts)
        check_results(case, run, (case.name, heap))
        assert run.counts["huge_search"] == 4 and run.counts["tail_retry"] == retries


def test_small_pools_send_search_items_to_the_tail_and_its_second_round_counts_a_read_without_final_state():
    """tandem(70, 2) (more copies than the instance lanes take) with large-capacity slots of 8 states: the boundary tasks and one
    more read — the same with another first base, 70 states until the last step and then none — are searched again by the last
    tier. With a heap of 64 KiB a slice holds 256 / 30 = 8 states: all of them are redone with the whole heap, where the read
    without a final state gets its read counter from the tail."""
    case = lc.tandem(70, 2, repeat=2, dead=True)
    dead = case.described[-2]
    assert dead[2] in (1, 2) and dead[6] is None  # (not exactly mapped: a missing k-mer, or no extension)
    roomy = Run(case, max_states=8, max_path_nodes=16)
    print(case.name, "default heap", roomy.counts)
    check_results(case, roomy, (case.name, "default heap"))
    assert roomy.counts["tail_retry"] == 0
    tight = Run(case, max_states=8, max_path_nodes=16, huge_heap_bytes=64 << 10)
    print(case.name, "64 KiB", tight.counts)
    check_results(case, tight, (case.name, "64 KiB"))
    assert tight.counts["huge_search"] == roomy.counts["huge_search"] == 6 and tight.counts["tail_retry"] == 6


def test_a_seed_wider_than_the_search_pools_is_handed_on_whole():
    """enc(20) without the instance lanes and with large-capacity slots of 8 states: the seed is ONE path-less interval over 20
    positions, which the large-capacity search takes apart position by position. The 9th does not fit: the task is the last
    tier's (huge_search), which records all 20 instances — not the first 8 (load_seed once ignored what its push answered for a
    plain seed: the task ended mapped with 8 final states, 8 candidates in its draw and n = 8 in its position record)."""
    case = lc.enc(20)
    run = Run(case, ("GMX_NO_INST",), max_states=8, max_path_nodes=16)
    base = Run(case, ("GMX_NO_INST",), with_boundary=False, max_states=8, max_path_nodes=16)
    print(case.name, run.counts)
    check_results(case, run, case.name)
    assert run.counts["huge_search"] - base.counts["huge_search"] == 2 and run.counts["inst_mapped"] == 0


# ---- 6: the switches over the same inputs ----------------------------------------------------------------------------------------
def family_cases():
    return [lc.enc(5), lc.enc(17), lc.enc(25), lc.sited_plus_plain(13), lc.sited_plus_plain(17), lc.tandem(2, 13), lc.tandem(2, 33),
            lc.tandem(5, 17), lc.tandem(17, 4), lc.tandem(25, 3), lc.chains((4, 5)), lc.chains((4, 4), plain=True),
            lc.chains((4,) * 11 + (5,), copies=2), lc.chains((5, 5, 4), plain=True, pad=True), lc.deep((9,)), lc.deep((33,)), lc.deep((25,), plain=True),
            lc.deep((12, 13)), lc.deep((16, 16, 17)), lc.deep((32, 33)), lc.members(((1,) * 11, (1,) * 11))]


ENVS = [("GMX_NO_COOP",), ("GMX_NO_COVER_ONE",), ("GMX_NO_COVER_JUMP",), ("GMX_NO_COOP", "GMX_NO_COVER_ONE"), ("GMX_NO_COOP", "GMX_NO_COVER_JUMP"),
        ("GMX_NO_COVER_ONE", "GMX_NO_COVER_JUMP")]


@pytest.mark.parametrize("env", ENVS, ids=["+".join(v[4:].lower() for v in e) for e in ENVS])
def test_switches_over_every_family(env):
    for case in family_cases():
        run = Run(case, env)
        print(case.name, env, run.counts)
        check_results(case, run, (case.name, env))
        if "GMX_NO_COOP" in env:
            assert run.counts["coop_rejected_general"] + run.counts["coop_rejected_inst"] + run.counts["coop_rejected_big"] == 0


def strand_expectation(case, limit):
    """Per strand, the oracle's coverage of the tasks of that orientation the limit does not leave out."""
    want = case.expectation(limit)
    out = []
    for strand in (0, 1):
        o = Oracle(case.prg, case.k)
        for t, (x, seed, code, multi, pos, n, what) in enumerate(case.described):
            if (t & 1) == strand and what is not None and t not in want["left_out"]:
                o.quasimap_read(x, seed)
        out.append(dict(allele_sum=o.allele_sum(), per_base={n["first_pos"]: n["cov"] for n in o.per_base_nodes()}))
        o.close()
    return out


RECORDED = [lambda: lc.enc(5), lambda: lc.enc(25), lambda: lc.tandem(2, 13), lambda: lc.tandem(17, 4), lambda: lc.deep((12, 13)),
            lambda: lc.deep((16, 16, 17)), lambda: lc.members(((1,) * 11, (1,) * 11))]


@pytest.mark.parametrize("env", [(), ("GMX_NO_COOP",)], ids=["coop", "serial"])
@pytest.mark.parametrize("i", range(len(RECORDED)))
def test_recordings_and_the_limit_on_candidates_on_every_tier(i, env):
    """record_strands, record_site_ambiguity and set_max_candidates(2): the tally and the left-out code differ per tier."""
    case = RECORDED[i]()
    run = Run(case, env, recordings=True, limit=2)
    print(case.name, env, run.counts)
    check_results(case, run, (case.name, env), limit=2)
    for got, want in zip(run.strands, strand_expectation(case, 2)):
        assert got["allele_sum"] == want["allele_sum"] and got["per_base"] == want["per_base"], (case.name, env)
    drawn, passed = sac.expect_from(case.prg, case.k, case.described, 2)
    assert (run.ambiguity[0][:drawn.size] == drawn).all() and (run.ambiguity[1][:passed.size] == passed).all(), (case.name, env)


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_cover_ladder as t
out = {}
for case in t.family_cases():
    for env in ((), ("GMX_NO_COOP",)):
        run = t.Run(case, env)
        try:
            t.check_results(case, run, case.name)
            ok = True
        except AssertionError as exc:
            ok = repr(exc)[:300]
        out[case.name + ("/serial" if env else "")] = dict(ok=ok, counts=run.counts)
print(json.dumps(out))
"""


@pytest.mark.parametrize("lanes", [16, 32, 5])
def test_cover_lanes(lanes):
    """GMX_COVER_LANES (the lane count, hence the LDS stride, of the one-lane LDS instances) is read once per process: one child
    per value, every family with and without the cooperative kernels in front, its verdict as JSON."""
    env = dict(os.environ, GMX_COVER_LANES=str(lanes))
    for v in SWITCHES:
        env.pop(v, None)
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    verdict = json.loads(out.stdout.strip().splitlines()[-1])
    print(verdict)
    assert all(v["ok"] is True for v in verdict.values()), {k: v for k, v in verdict.items() if v["ok"] is not True}
    assert sum(v["counts"]["mid"] for v in verdict.values()) > 0 and sum(v["counts"]["overflow"] for v in verdict.values()) > 0

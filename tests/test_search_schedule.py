"""The search schedule carries no semantics: how many wave-loop iterations a task gets before the probe or the extend kernel
parks it (GMX_PROBE_ITERS, GMX_EXTEND_BUDGET), whether transitions are fused (GMX_NO_FUSE), how many straggler passes follow
(GMX_EXTEND_PASSES), whether the last one runs under a cap and hands the rest to the split search (GMX_EXTEND_CAP), and which
tiers exist (GMX_NO_INST, GMX_NO_SPLIT2) only decide WHERE a task's search is interrupted and resumed. Moving the park point
over budgets 1, 2, 3, ... puts it on every kind of lane state and every stack depth; every placement must give the oracle's
coverage, read counters and final states, and the per-read logs of the default schedule.

Each case is one engine created under its variables and one launch of a small fixed-seed input (tests/schedule_common.py).
Every case also proves, from the queue counters and gmx_debug_straggler_counts, that its route was taken: without that the
comparison would be vacuous."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from schedule_common import Run, get_input, mixed_case, reference_run
from oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

NESTED = ("N", "N16", "N40")


def check_results(inp, run, note):
    """Checks 1-3 of a run: coverage and read counters against the oracle, per-task final states against the oracle (at most the
    tasks of the heap-backed tier keep none), per-read logs against the default schedule's."""
    print(note, inp.name, run.counts())
    assert run.cov == inp.want_cov, note
    if inp.states:
        assert not run.bad_states, (note, run.bad_states[:5])
        assert run.n_ecap <= run.q["huge_search"], (note, run.n_ecap, run.q)
    if inp.logs:
        ref = reference_run(inp.name)
        assert run.outcomes.shape == ref.outcomes.shape and run.positions.shape == ref.positions.shape
        bad = np.flatnonzero(run.outcomes != ref.outcomes)
        assert bad.size == 0, (note, [(int(i), int(run.outcomes[i]), int(ref.outcomes[i])) for i in bad[:10]])
        bad = np.flatnonzero((run.positions != ref.positions).any(axis=1))
        assert bad.size == 0, (note, [(int(i), run.positions[i].tolist(), ref.positions[i].tolist()) for i in bad[:10]])


def ids(envs):
    return ["-".join(f"{k[4:].lower()}={v}" for k, v in e.items()) or "default" for e in envs]


# ---- the inputs themselves: nothing here needs a GPU -------------------------------------------------------------------
def test_inputs_meet_their_conditions_on_the_host():
    """Input construction and the oracle's side of every expectation. On F a mapped task of >= 100 bases exists: behind a seed
    of <= 15 bases it has >= 85 left, one text iteration consumes at most one 64-symbol record, so it needs at least two
    iterations of the wave loop and a budget of 1 must park it."""
    f = get_input("F")
    assert len(f.reads) == 700 and min(len(r) for r in f.reads) >= 100
    assert any((r == 0).any() for r in f.reads[600:]), "no read with an N"
    assert f.index.info.kmer_size2 > f.k > 0
    assert f.want_cov["stats"]["exact_mapped"] > 600 and f.want_cov["stats"]["skipped"] > 0
    o = Oracle(f.prg, f.k, all_kmers=True)
    assert any(len(r) >= 100 and (o.search_read_backwards(r) or o.search_read_backwards(o.reverse_complement(r))) for r in f.reads[:8])
    o.close()
    for name in NESTED + ("C",):
        inp = get_input(name)
        assert inp.want_cov["stats"]["exact_mapped"] >= len(inp.reads)
    for name in NESTED:
        inp = get_input(name)
        assert inp.index.info.kmer_size2 > inp.k
        mapped = [w for pair in inp.want_states for w in pair if w]
        assert len(mapped) >= len(inp.reads)
        assert max(len(w) for w in mapped) > 1, "no task with several final instances"
    for name in ("F",) + NESTED:  # the oracle's per-read records: a byte and four words per read
        want_bytes, want_records = get_input(name).want_logs
        assert want_bytes.shape == (len(get_input(name).reads),) and want_records.shape == (len(get_input(name).reads), 4)
    for seed in range(12):
        inp, env = mixed_case(seed)
        assert env and len(inp.reads) > 50 and all(20 <= len(r) <= 60 for r in inp.reads)
        assert inp.want_cov["stats"]["exact_mapped"] > 0


def test_the_straggler_counts_hook_is_declared_guarded_and_bound():
    import re
    from gramtools_amd import Quasimapper, _lib
    header = open(os.path.join(ROOT, "include", "gmx.h")).read()
    assert re.search(r"\bint\s+gmx_debug_straggler_counts\(gmx_engine \*e, uint64_t out\[3\]\);", header)
    source = open(os.path.join(ROOT, "gramtools_amd", "csrc", "gmx_engine_readback.h")).read()
    assert re.search(r"int gmx_debug_straggler_counts\([^)]*\) try \{.*?\} GMX_GUARD_INT\(\"gmx_debug_straggler_counts\"\)", source, re.S)
    assert hasattr(_lib.load(), "gmx_debug_straggler_counts") and callable(Quasimapper.debug_straggler_counts)


# ---- default schedule: the references the cases below are compared with ------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["F", "N", "N16", "N40", "C", "R17", "R70", "Nsmall"])
def test_default_schedule(name):
    inp = get_input(name)
    run = reference_run(name)
    check_results(inp, run, "default")
    if name != "Nsmall":
        assert run.q["huge_search"] == 0 and run.n_ecap == 0, run.q
    if name == "C":
        assert run.q["seed_cursor"] == 1
    if name == "R17":  # the issue's R: one input that crosses both tiers (measured: inst_mapped 111, overflow_probe 257)
        assert run.q["inst_mapped"] > 0 and run.q["overflow_extend"] + run.q["overflow_probe"] > 0, run.q
    if name == "R70":
        assert run.q["overflow_extend"] + run.q["overflow_probe"] > 0 and run.q["big_mapped"] > 0, run.q
    if name == "Nsmall":  # what GMX_NO_SPLIT2 takes away exists by default
        assert run.q["overflow_split"] > 0, run.q


@gpu
@pytest.mark.parametrize("name", ("F",) + NESTED + ("Nsmall",))
def test_default_logs_are_the_oracles(name):
    """The records the other cases are compared with, against the oracle's own (tests/test_read_outcomes.py,
    tests/test_read_positions.py)."""
    inp, run = get_input(name), reference_run(name)
    want_bytes, want_records = inp.want_logs
    assert (run.outcomes == want_bytes).all()
    assert (run.positions == want_records).all()


# ---- extend budget -----------------------------------------------------------------------------------------------------
EXTEND = [dict({"GMX_EXTEND_BUDGET": str(b)}, **({"GMX_NO_FUSE": "1"} if nf else {})) for b in (0, 1, 2, 3, 5, 13) for nf in (0, 1)]


@gpu
@pytest.mark.parametrize("env", EXTEND, ids=ids(EXTEND))
@pytest.mark.parametrize("name", ["F", "N", "N16", "N40", "C"])
def test_extend_budget(name, env):
    inp = get_input(name)
    run = Run(inp, env)
    check_results(inp, run, env)
    budget = int(env["GMX_EXTEND_BUDGET"])
    if budget in (1, 2, 3):
        assert run.stragglers[0] > 0, run.counts()
    if budget == 0:
        assert run.stragglers == [0, 0, 0], run.counts()
    if name == "C":
        assert run.q["seed_cursor"] == 1


@gpu
def test_parking_loses_no_task_and_counts_none_twice():
    """F, default schedule against no budget at all: the same number of tasks leaves the search mapped."""
    a, b = reference_run("F"), Run(get_input("F"), {"GMX_EXTEND_BUDGET": "0"})
    total = lambda q: q["mapped"] + q["big_mapped"] + q["inst_mapped"]
    assert total(a.q) == total(b.q) > 0, (a.counts(), b.counts())
    assert total(a.q) == get_input("F").want_cov["stats"]["exact_mapped"]


# ---- probe budget ------------------------------------------------------------------------------------------------------
PROBE = [dict({"GMX_NO_SEEDED": "1", "GMX_PROBE_ITERS": str(p)}, **({"GMX_EXTEND_BUDGET": "1"} if eb else {})) for p in (0, 1, 2, 4)
         for eb in (0, 1)]


@gpu
@pytest.mark.parametrize("env", PROBE, ids=ids(PROBE))
@pytest.mark.parametrize("name", ["F", "N", "N16", "N40", "C"])
def test_probe_budget(name, env):
    inp = get_input(name)
    run = Run(inp, env)
    check_results(inp, run, env)
    if env["GMX_PROBE_ITERS"] == "1":
        # (measured: every input gives stragglers — F 355, N 392, N16 104, N40 149, C 259 with the default extend budget —
        #  and only N40 a probe overflow as well, one task)
        assert run.q["alive"] > 0, run.counts()
        assert run.q["overflow_probe"] > 0 or sum(run.stragglers) > 0, run.counts()
    if env.get("GMX_EXTEND_BUDGET") == "1":
        assert run.stragglers[0] > 0, run.counts()


# ---- straggler passes --------------------------------------------------------------------------------------------------
PASSES = [{"GMX_EXTEND_BUDGET": "1", "GMX_EXTEND_PASSES": p} for p in ("1", "1,1", "2,3")]


@gpu
@pytest.mark.parametrize("env", PASSES, ids=ids(PASSES))
@pytest.mark.parametrize("name", ["F", "N", "N16", "N40"])
def test_straggler_passes(name, env):
    inp = get_input(name)
    run = Run(inp, env)
    check_results(inp, run, env)
    assert run.stragglers[0] > 0, run.counts()
    if env["GMX_EXTEND_PASSES"] != "1":
        assert run.stragglers[1] > 0, run.counts()
    if env["GMX_EXTEND_PASSES"] == "1,1":
        assert run.stragglers[2] > 0, run.counts()


# ---- the capped last pass ----------------------------------------------------------------------------------------------
CAPS = [dict({"GMX_EXTEND_BUDGET": "1", "GMX_EXTEND_CAP": str(c)}, **({"GMX_EXTEND_PASSES": "1,1"} if p else {})) for c in (1, 3) for p in (0, 1)]


@gpu
@pytest.mark.parametrize("env", CAPS, ids=ids(CAPS))
@pytest.mark.parametrize("name", ["F", "N", "N16", "N40"])
def test_capped_last_pass(name, env):
    """What the cap cuts off goes to the split search and the large slot: more overflows than the same schedule without it."""
    inp = get_input(name)
    run = Run(inp, env)
    check_results(inp, run, env)
    uncapped = reference_run(name, tuple(sorted((k, v) for k, v in env.items() if k != "GMX_EXTEND_CAP")))
    assert run.q["overflow_extend"] > 0 and run.q["overflow_extend"] > uncapped.q["overflow_extend"], (run.counts(), uncapped.counts())
    assert run.stragglers[0] > 0


# ---- tiers -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["R17", "R70", "N", "N16", "N40"])
def test_without_instance_lanes(name):
    inp = get_input(name)
    run = Run(inp, {"GMX_NO_INST": "1"})
    check_results(inp, run, "GMX_NO_INST")
    assert run.q["inst_mapped"] == 0, run.counts()
    if name == "R17":  # (the one input whose default run has instance lanes: 111 tasks; on the others the knob only must not hurt)
        ref = reference_run(name)
        assert ref.q["inst_mapped"] > 0
        assert run.q["big_mapped"] == ref.q["big_mapped"] + ref.q["inst_mapped"], (run.counts(), ref.counts())


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from schedule_common import Run, get_input
out = {}
for name in sys.argv[2:]:
    inp = get_input(name)
    run = Run(inp, {})
    out[name] = dict(cov=run.cov == inp.want_cov, bad_states=len(run.bad_states), n_ecap=run.n_ecap, counts=run.counts(),
                     logs=run.logs_equal_the_oracles(inp) if inp.logs else None)
print(json.dumps(out))
"""


@gpu
def test_without_the_second_split_search():
    """GMX_NO_SPLIT2 is read once per process: one child, all inputs, its verdict as JSON."""
    names = ["R17", "R70", "N", "N16", "N40", "Nsmall"]
    env = dict(os.environ, GMX_NO_SPLIT2="1")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT] + names, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    verdict = json.loads(out.stdout.strip().splitlines()[-1])
    print(verdict)
    for name in names:
        v = verdict[name]
        assert v["cov"] and v["bad_states"] == 0 and v["n_ecap"] <= v["counts"]["huge_search"], (name, v)
        assert v["logs"] is (True if get_input(name).logs else None), (name, v)
        assert v["counts"]["overflow_split"] == 0, (name, v)
    assert verdict["R70"]["counts"]["big_mapped"] > 0, verdict["R70"]
    # the knob took something away: by default Nsmall's split search hands tasks on, and they end in the same large slots
    ref = reference_run("Nsmall")
    assert ref.q["overflow_split"] > 0, ref.counts()
    assert verdict["Nsmall"]["counts"]["big_mapped"] == ref.q["big_mapped"] > 0, (verdict["Nsmall"], ref.counts())


# ---- mixed -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", range(12))
def test_mixed_schedules_on_random_prgs(seed):
    inp, env = mixed_case(seed)
    base = Run(inp, {k: v for k, v in env.items() if k == "GMX_SEED_CURSOR"})
    assert base.q["huge_search"] == 0 and base.cov == inp.want_cov and not base.bad_states, (base.counts(), base.bad_states[:5])
    run = Run(inp, env)
    check_results(inp, run, env)
    # the route was taken, from the case's own variables
    budget, passes = int(env["GMX_EXTEND_BUDGET"]), env.get("GMX_EXTEND_PASSES")
    if budget in (1, 2, 3):
        assert run.stragglers[0] > 0, run.counts()
    if passes:
        assert run.stragglers[0] > 0 and run.stragglers[1] > 0, run.counts()
    if passes == "1,1":
        assert run.stragglers[2] > 0, run.counts()
    if "GMX_EXTEND_CAP" in env:
        uncapped = Run(inp, {k: v for k, v in env.items() if k != "GMX_EXTEND_CAP"})
        assert run.q["overflow_extend"] > 0 and run.q["overflow_extend"] > uncapped.q["overflow_extend"], (run.counts(), uncapped.counts())
    if env.get("GMX_PROBE_ITERS") == "1":
        assert run.q["alive"] > 0 and (run.q["overflow_probe"] > 0 or sum(run.stragglers) > 0), run.counts()
    if "GMX_NO_INST" in env:
        assert run.q["inst_mapped"] == 0, run.counts()

"""Inputs, oracle expectations and the one-launch runner of tests/test_search_schedule.py (shared with its child process).

Every input is small and fixed-seed, and everything the oracle says about it is computed once per process:
  F        flat, 6 kb, 150 mixed sites, k = 7 (a longer seed table: the seeded pipeline; GMX_NO_SEEDED=1: the probe pipeline),
           600 error-free reads of 100-150 bases and 100 reads with substitutions, Ns and ragged ends (tasks that die mid-read)
  N, N16, N40   nested low-complexity PRGs, k = 5, reads of 30, 16 and 40 bases: many states per task, so the stack is not empty
           when a task is parked
  C        a dense nested PRG at k = 4 under GMX_SEED_CURSOR=1: seed entries taken state by state across park and resume
  Nsmall   N with large-capacity slots of 64 states and 128 path nodes: the split search hands tasks on (overflow_split > 0)
  R17, R70 the repeats of tests/test_repeats.py at their smallest useful size: 17 copies (one lane per mapping instance),
           70 copies (the overflow queues and the split search)"""
import functools

import numpy as np
import pytest

from common import canonical_cov, flatten_reads, oracle_map
from gramtools_amd import Index, Quasimapper, master_seeds
from gramtools_amd.synth import (bracket_to_ints, mixed_variant_prg, nested_prg, random_ref, realistic_reads, simulate_graph_reads,
                                 simulate_haplotype_reads, split_reads)
from oracle import Oracle
from states_common import encapsulated_instances, instances
from test_repeats import _repeat_workload

# every variable of the search schedule: a run starts from none of them
SCHEDULE_VARS = ("GMX_EXTEND_BUDGET", "GMX_PROBE_ITERS", "GMX_NO_FUSE", "GMX_EXTEND_PASSES", "GMX_EXTEND_CAP", "GMX_NO_INST",
                 "GMX_NO_SEEDED", "GMX_SEED_CURSOR")


class Input:
    def __init__(self, name, prg, k, reads, base_env=None, states=False, logs=False, engine_kw=None):
        self.name, self.prg, self.k = name, prg, k
        self.engine_kw = dict(engine_kw or {})  # capacities of the engine (Quasimapper's keywords)
        self.reads = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
        self.flat, self.offs = flatten_reads(self.reads)
        self.seeds = master_seeds(42, [len(self.reads)])
        self.base_env = dict(base_env or {})
        self.states, self.logs = states, logs  # which of the per-task checks a run of this input carries

    @functools.cached_property
    def index(self):
        return Index(self.prg, self.k)

    @functools.cached_property
    def want_cov(self):
        return oracle_map(self.prg, self.k, (self.flat, self.offs), self.seeds, threads=8)

    @functools.cached_property
    def want_states(self):
        """[read][orientation] -> the oracle's search_read_backwards, as instances"""
        o = Oracle(self.prg, self.k, all_kmers=True)
        out = [[instances(o.search_read_backwards(o.reverse_complement(r) if ori else r)) for ori in (0, 1)] for r in self.reads]
        o.close()
        return out

    @functools.cached_property
    def want_logs(self):
        """(outcome bytes, position records) from the oracle's own steps: the expectations of tests/test_read_outcomes.py and
        tests/test_read_positions.py as they stand"""
        from test_read_outcomes import oracle_bytes
        from test_read_positions import oracle_records
        return oracle_bytes(self.prg, self.k, self.reads)[0], oracle_records(self.prg, self.k, self.reads, self.seeds)[0]


def _flat():
    ref = random_ref(6000, 3)
    prg, sites = mixed_variant_prg(ref, 150, 4, max_alleles=4)
    reads = simulate_haplotype_reads(ref, sites, 600, 100, 150, 5)
    whole = np.stack(simulate_haplotype_reads(ref, sites, 100, 150, 150, 6))
    flat, offs = realistic_reads(whole, 7, sub_rate=0.01, n_read_frac=0.05, len_lo=100)
    return Input("F", prg, 7, reads + [np.array(r) for r in split_reads(flat, offs)], logs=True)


def _nested(name, seed, n_reads, read_len, **engine_kw):
    prg = bracket_to_ints(nested_prg(seed, n_top=10, max_depth=3).replace("t", "a"))
    return Input(name, prg, 5, simulate_graph_reads(prg, n_reads, read_len, seed), states=True, logs=True, engine_kw=engine_kw)


def _cursor():
    prg = bracket_to_ints(nested_prg(41, n_top=10, max_depth=3).replace("t", "a"))  # (tests/test_seed_units.py, _nested_case(1))
    return Input("C", prg, 4, simulate_graph_reads(prg, 300, 24, 1), base_env={"GMX_SEED_CURSOR": "1"})


def _repeats(name, copies):
    prg, reads = _repeat_workload(40000, 500, 1200, 40 + copies, copies=copies - 1, seg=600)
    return Input(name, prg, 8, list(reads))


_MAKERS = {"F": _flat, "N": lambda: _nested("N", 91, 400, 30), "N16": lambda: _nested("N16", 92, 150, 16),
           "N40": lambda: _nested("N40", 93, 150, 40), "C": _cursor,
           # N with small large-capacity slots: a group's parts of a slot do not suffice under the 16-lane split search
           "Nsmall": lambda: _nested("Nsmall", 91, 400, 30, max_states=64, max_path_nodes=128), "R17": lambda: _repeats("R17", 17),
           "R70": lambda: _repeats("R70", 70)}


@functools.lru_cache(maxsize=None)
def get_input(name):
    return _MAKERS[name]()


@functools.lru_cache(maxsize=None)
def mixed_case(seed):
    """A random nested or flat PRG as tests/test_gpu_states.py draws its own, with reads of 20-60 bases, and a random schedule."""
    rng = np.random.default_rng(1000 + seed)
    L, k = int(rng.integers(20, 61)), int(rng.integers(2, 6))
    if seed % 2 == 0:
        s = nested_prg(200 + seed, n_top=int(rng.integers(10, 16)), max_depth=int(rng.integers(1, 4)), seq_max=int(rng.integers(3, 8)))
        if seed % 3 == 0:  # low-complexity PRGs: repeats, many states per read
            s = s.replace("t", "a").replace("g", "c")
        prg = bracket_to_ints(s)
        reads = simulate_graph_reads(prg, 60, L, seed + 100)
    else:
        ref = random_ref(int(rng.integers(300, 1200)), 200 + seed)
        prg, sites = mixed_variant_prg(ref, int(rng.integers(10, 40)), seed, max_alleles=4)
        reads = simulate_haplotype_reads(ref, sites, 60, 20, L, seed + 100)
    reads += [rng.integers(1, 5, size=L).astype(np.uint8) for _ in range(6)]
    env = {}
    if rng.random() < 0.5:
        env["GMX_NO_SEEDED"] = "1"
        env["GMX_PROBE_ITERS"] = str(int(rng.choice([0, 1, 2, 4])))
    env["GMX_EXTEND_BUDGET"] = str(int(rng.choice([1, 1, 2, 3, 5])))
    if rng.random() < 0.5:
        env["GMX_NO_FUSE"] = "1"
    if rng.random() < 0.5:
        env["GMX_EXTEND_PASSES"] = str(rng.choice(["1", "1,1", "2,3"]))
    if rng.random() < 0.35:
        env["GMX_EXTEND_CAP"] = str(int(rng.choice([1, 3])))
    if rng.random() < 0.25:
        env["GMX_NO_INST"] = "1"
    if rng.random() < 0.3:
        env["GMX_SEED_CURSOR"] = "1"
    return Input("mixed%d" % seed, prg, k, [r for r in reads if len(r) >= 20], states=True), env


class Run:
    """What one engine under one schedule left after one launch."""

    def __init__(self, inp, env, keep_engine=False):
        with pytest.MonkeyPatch.context() as mp:
            for v in SCHEDULE_VARS:
                mp.delenv(v, raising=False)
            for name, value in {**inp.base_env, **env}.items():
                mp.setenv(name, value)
            qm = Quasimapper(inp.index, **inp.engine_kw)
            if inp.states:
                qm.debug_keep_states()
            if inp.logs:
                qm.record_outcomes()
                qm.record_positions()
            qm.map_reads(inp.flat, inp.offs, inp.seeds)
            self.cov = canonical_cov(qm.coverage())
            self.q = qm.queue_counts()
            self.stragglers = qm.debug_straggler_counts()
            self.outcomes = qm.outcomes() if inp.logs else None
            self.positions = qm.positions() if inp.logs else None
            self.bad_states, self.n_ecap = self._compare_states(inp, qm) if inp.states else ([], 0)
            self.qm = qm if keep_engine else None
            if not keep_engine:
                qm.close()

    @staticmethod
    def _compare_states(inp, qm):
        """Every (read, orientation): the task's final states against the oracle's. -> (mismatches, tasks that answered GMX_ECAP:
        the heap-backed tier keeps no states)"""
        bad, n_ecap = [], 0
        for i in range(len(inp.reads)):
            for ori in (0, 1):
                try:
                    states, tier = qm.debug_final_states(i, ori)
                except Exception as exc:
                    if getattr(exc, "code", None) != -4:
                        raise
                    n_ecap += 1
                    continue
                got = encapsulated_instances(qm, states)
                if got != inp.want_states[i][ori]:
                    bad.append((i, ori, tier, got[:4], inp.want_states[i][ori][:4]))
        return bad, n_ecap

    def logs_equal_the_oracles(self, inp):
        want_bytes, want_records = inp.want_logs
        return bool((self.outcomes == want_bytes).all() and (self.positions == want_records).all())

    def counts(self):
        q = self.q
        return dict(stragglers=self.stragglers, alive=q["alive"], overflow_probe=q["overflow_probe"], overflow_extend=q["overflow_extend"],
                    overflow_split=q["overflow_split"], mapped=q["mapped"], big_mapped=q["big_mapped"], inst_mapped=q["inst_mapped"],
                    huge_search=q["huge_search"])


@functools.lru_cache(maxsize=None)
def reference_run(name, env_items=()):
    """The run of an input under a schedule other runs are compared with (the default one: no variable set), once per process."""
    return Run(get_input(name), dict(env_items))

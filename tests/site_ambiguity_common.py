"""Per-site ambiguity counts (gmx_engine_record_site_ambiguity): the expectation shared by test_site_ambiguity.py
(GPU) and test_site_ambiguity_host.py. It comes from the oracle alone, task by task over max_candidates_common.describe_tasks:

  drawn   a second Oracle receives quasimap_read(x, seed) only for the AMBIGUOUS tasks (a class and more than one candidate) the
          limit does not leave out; drawn[s] is the sum of that oracle's grouped counts at site s (a task adds one grouped count
          to every site its drawn class records at, none when its draw falls on the non-variant instances).
  passed  for the ambiguous tasks that are left out, or whose draw r falls on the non-variant instances (r <= nonvar): the level-0
          site sets of unique_site_paths' entries, +1 per entry per site."""
import functools

import numpy as np

from oracle import Oracle
from oracle.oracle import RNG_LEMIRE
import max_candidates_common as mc
from max_candidates_common import total_of


def is_ambiguous(what):
    return total_of(what) > 1


def expect_from(prg, k, described, limit, seeds_of=None, mode=RNG_LEMIRE):
    """(drawn, passed) as uint32 arrays under `limit` (0: none). seeds_of: per task, a seed in place of the described one."""
    o, second = Oracle(prg, k, rng_mode=mode), Oracle(prg, k, rng_mode=mode)
    n_sites = o.num_sites()
    passed = np.zeros(n_sites, dtype=np.uint32)
    for t, (x, seed, code, multi, pos, n, what) in enumerate(described):
        if not is_ambiguous(what):
            continue
        if seeds_of is not None:
            seed = int(seeds_of[t])
        total = total_of(what)
        left = bool(limit) and total > limit
        r = 0 if left else int(Oracle.rng_generate(seed, 1, total, 1, mode)[0])
        if left or r <= what["nonvar"]:
            nonvar, entries = o.unique_site_paths(o.search_read_backwards(x))
            assert nonvar == what["nonvar"] and len(entries) == what["classes"]
            for sites, _, _ in entries:
                for marker in sites:
                    passed[(marker - 5) >> 1] += 1
        if not left:
            second.quasimap_read(x, seed)
    drawn = np.asarray([sum(site.values()) for site in second.grouped()], dtype=np.uint32)
    assert drawn.size == n_sites
    o.close()
    second.close()
    return drawn, passed


@functools.lru_cache(maxsize=None)
def expectation(name, limit):
    prg, k, _, _ = mc.case(name)
    return expect_from(prg, k, mc.described(name), limit)


def n_ambiguous(name):
    return sum(1 for d in mc.described(name) if is_ambiguous(d[6]))

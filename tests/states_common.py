"""SearchStates as order-insensitive sets of mapping instances: a state over [lo, hi] stands for hi - lo + 1 instances
(SA index, traversed path, traversing path). The reference merges neighbouring instances of one allele into an interval
(encapsulated_search.cpp:64-85) and the device keeps single positions in text form; the instances are the same.
Shared by tests/test_gpu_states.py and tests/test_search_schedule.py."""


def instances(states):
    out = []
    for s in states:
        lo, hi = int(s[0]), int(s[1])
        tvd = tuple((int(m), int(a)) for m, a in (s[2] if len(s) > 2 else []))
        tvg = tuple(int(x[0]) for x in (s[3] if len(s) > 3 else []))
        out += [(i, tvd, tvg) for i in range(lo, hi + 1)]
    return sorted(out)


def encapsulated_instances(qm, states):
    """the device's handle_allele_encapsulated_states on `states`, as instances"""
    if not states:
        return []
    inside, outside = qm.debug_encapsulate(states)
    return sorted(instances(inside) + [(i, (), ()) for i in outside])

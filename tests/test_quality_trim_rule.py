"""The quality-trimming rule (gmx_qtrim.h, exported as gmx_quality_trim_length): the running sum of `bwa aln -q` and cutadapt `-q`
over Phred+33 qualities, 3' end only — against a restatement of the rule in Python, on random and on crafted quality strings.
No GPU: this is the host's compilation of the text the device's record scan compiles too (tests/test_quality_trim_device.py)."""
import numpy as np
import pytest


def trim_ref(qual: bytes, Q: int) -> int:
    """t for the quality bytes `qual` at threshold Q: the read keeps bases [0, t)."""
    n = len(qual)
    s, best, t = 0, 0, n
    for i in range(n - 1, -1, -1):
        s += Q - max(qual[i] - 33, 0)
        if s < 0:
            break
        if s > best:
            best, t = s, i
    return t


def phred(qs) -> bytes:
    return bytes(33 + q for q in qs)


def test_random_strings_agree_with_the_restated_rule():
    from gramtools_amd import quality_trim_length
    rng = np.random.default_rng(2024)
    n_cases = 0
    for i in range(2000):
        n = int(rng.integers(0, 81))
        # three kinds of string: any quality, good with a poor tail, values around the thresholds
        kind = i % 3
        if kind == 0:
            q = rng.integers(0, 94, n)
        elif kind == 1:
            q = np.concatenate([rng.integers(25, 42, n - n // 3), rng.integers(0, 30, n // 3)])
        else:
            q = rng.choice([0, 1, 2, 3, 19, 20, 21, 29, 30, 31, 92, 93], n)
        qual = phred(int(x) for x in q)
        for Q in (1, 2, 20, 30, 93):
            assert quality_trim_length(qual, Q) == trim_ref(qual, Q), (list(q), Q)
            n_cases += 1
    assert n_cases == 10000


@pytest.mark.parametrize("qs,Q,t", [
    ([40] * 30, 20, 30),                    # all high: nothing goes
    ([2] * 30, 20, 0),                      # all low: everything goes
    ([40] * 29 + [2], 20, 29),              # one low last base
    ([40] * 5 + [10, 25, 10], 20, 5),       # s = 10, 5, 15: the good base in the poor tail goes too (a trailing-threshold trimmer says 7)
    ([40, 10, 30, 10], 20, 3),              # s = 10, 0, 10: a tie keeps the longer read
    ([20] * 12, 20, 12),                    # q == Q removes nothing
    ([40, 40, 20, 20], 20, 4),              # ... also behind good bases (s stays 0)
    ([], 20, 0),
    ([5], 20, 0),
    ([50], 20, 1),
])
def test_crafted_cases(qs, Q, t):
    from gramtools_amd import quality_trim_length
    assert trim_ref(phred(qs), Q) == t  # (the restatement itself, on cases worked out by hand)
    assert quality_trim_length(phred(qs), Q) == t


def test_bytes_below_33_count_as_quality_0():
    from gramtools_amd import quality_trim_length
    good = phred([40] * 10)
    for low in (0, 10, 32, 33):  # 32 is what a BAM record without qualities arrives as
        qual = good + bytes([low] * 4)
        assert quality_trim_length(qual, 20) == trim_ref(qual, 20) == 10
    assert quality_trim_length(bytes([32] * 25), 1) == 0
    # q = 0 throughout cannot be told from q = 0 by a lower byte: the sums are equal
    assert quality_trim_length(bytes([0] * 7) + good, 20) == 17


def test_threshold_0_keeps_the_read():
    from gramtools_amd import quality_trim_length
    rng = np.random.default_rng(1)
    for n in (0, 1, 33, 80):
        assert quality_trim_length(phred(int(x) for x in rng.integers(0, 94, n)), 0) == n

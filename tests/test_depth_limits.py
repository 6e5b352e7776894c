"""uint16 semantics under real depth: more than 65 536 reads over one small site. The reference's
counters are uint16: allele-sum and grouped counts wrap (data_types.hpp:52), per-base saturates at 65535
(allele_base.cpp:239). The engine accumulates uint32 on the device and applies both as functions of the total, so
it must equal the oracle (which counts in uint16 like the reference) — also when the reads arrive in two calls.

This file is one engine and one two-allele site with dense counters (the hit-counter path). Totals that pass 65 535 only when
they are ADDED — by an exchange between engines or ranks, by the two strands' blocks, by the grouped log's counted records — and
the read counters' 16-bit limbs up to 2^64 are in test_depth_exchange.py (GPU) and test_depth_exchange_host.py (no GPU), on the
case of depth_common.py."""
import numpy as np
import pytest

from gramtools_amd import Index, Quasimapper, master_seeds
from oracle.prg_text import encode_prg

from common import canonical_cov, flatten_reads, hostemu_map, oracle_map


def _deep_reads(n):
    # PRG  acgtacgtt[a,g]ccatg : reads over the site carrying allele 'a' (70 %) or 'g' (30 %), both strands
    a = np.array([1, 2, 3, 4, 4, 1, 2, 2, 1], dtype=np.uint8)       # a c g t t A c c a
    g = np.array([1, 2, 3, 4, 4, 3, 2, 2, 1], dtype=np.uint8)
    rng = np.random.default_rng(1)
    reads = []
    for i in range(n):
        r = a if rng.random() < 0.7 else g
        reads.append(r if i % 2 == 0 else (5 - r[::-1]).astype(np.uint8))
    return reads


def test_host_emulation_wraps_and_saturates_like_the_oracle():
    prg = encode_prg("acgtacgtt5a6g6ccatg")
    reads = _deep_reads(140000)
    seeds = master_seeds(3, [len(reads)])
    want = oracle_map(prg, 3, reads, seeds, threads=1)
    got, _, rc = hostemu_map(prg, 3, reads, seeds)
    assert rc == 0 and got == want
    assert any(v == 65535 for site in want["per_base"].values() for v in site)   # saturated
    assert sum(want["allele_sum"][0]) < 140000                                      # wrapped


@pytest.mark.gpu
def test_gpu_wraps_and_saturates_like_the_oracle():
    prg = encode_prg("acgtacgtt5a6g6ccatg")
    reads = _deep_reads(140000)
    seeds = master_seeds(3, [len(reads)])
    want = oracle_map(prg, 3, reads, seeds, threads=1)
    qm = Quasimapper(Index(prg, 3))
    half = len(reads) // 2
    for part, sd in ((reads[:half], seeds[:half]), (reads[half:], seeds[half:])):
        flat, offs = flatten_reads(part)
        qm.map_reads(flat, offs, sd)
    assert canonical_cov(qm.coverage()) == want

"""The limit on a selection's candidates (gmx_engine_set_max_candidates), the parts that need no GPU: the three cases
meet, through the oracle, the counts they were built for; the expectation with the limit off is the oracle's own map_reads; the
entry points are declared, exported, guarded and mirrored in gramtools_amd/_lib.py; `gram genotype` refuses a bad value before
it creates an engine."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import oracle_map
from gramtools_amd import _lib, Quasimapper, QuasimapperGroup
from max_candidates_common import allele_sum_total, case, described, expectation, total_of, without_stats
from test_read_outcomes_host import declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gramtools_amd", "csrc")
NEW = ("gmx_engine_set_max_candidates", "gmx_engine_max_candidates", "gmx_group_set_max_candidates")
CTYPE = {"int": C.c_int, "uint32_t": C.c_uint32, "gmx_engine *": C.c_void_p, "gmx_group *": C.c_void_p}


def totals(name):
    """How many tasks of the case have which range of the draw (tasks without a class left aside)."""
    return collections.Counter(t for t in (total_of(d[6]) for d in described(name)) if t)


def left_out(name, limit):
    return len(expectation(name, limit)["left_out"])


def test_ladder_meets_its_counts():
    prg, k, reads, _ = case("ladder")
    assert len(prg) == 1708 and k == 6 and len(reads) == 400 and len(described("ladder")) == 800
    hist = totals("ladder")
    assert sum(hist.values()) == 145
    assert set(hist) == {1, 2, 3, 4, 5, 7, 8} and all(n >= 10 for n in hist.values()), hist
    assert [left_out("ladder", L) for L in (1, 2, 3, 5, 8)] == [128, 117, 103, 58, 0]
    assert [allele_sum_total(expectation("ladder", L)["cov"]) for L in (0, 1, 2, 3, 5, 8)] == [145, 17, 28, 42, 87, 145]


def test_nested_ladder_meets_its_counts():
    prg, k, reads, _ = case("nested_ladder")
    assert len(prg) == 928 and k == 5 and len(reads) == 400 and int(max(prg) - 3) // 2 == 22
    hist = totals("nested_ladder")
    assert sum(hist.values()) == 177 and set(hist) == {1, 2, 3, 4, 5}, hist
    assert [left_out("nested_ladder", L) for L in (1, 2, 3, 5)] == [128, 84, 66, 0]


def test_half_sited_counts_the_non_variant_instances_toward_the_total():
    ten = [d[6] for d in described("half_sited") if total_of(d[6]) == 10]
    assert len(ten) == 55 and all(w["nonvar"] == 5 and w["classes"] == 5 for w in ten)
    assert totals("half_sited") == {10: 55}
    assert left_out("half_sited", 9) == 55 and allele_sum_total(expectation("half_sited", 9)["cov"]) == 0
    assert left_out("half_sited", 10) == 0 and allele_sum_total(expectation("half_sited", 10)["cov"]) == 28


@pytest.mark.parametrize("name", ["ladder", "nested_ladder", "half_sited"])
def test_the_expectation_without_a_limit_is_the_oracles_own_mapping(name):
    prg, k, reads, seeds = case(name)
    e = expectation(name, 0)
    assert e["left_out"] == [] and not (e["bytes"] & 0xC0).any()
    assert e["cov"] == without_stats(oracle_map(prg, k, list(reads), seeds))


def test_the_entry_points_are_declared_exported_and_guarded():
    lib = C.CDLL(_lib.LIB) if os.path.exists(_lib.LIB) else _lib.load()
    text = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp")))
    guarded = set(re.findall(r'GMX_GUARD_(?:INT|VOID|PTR|ZERO)\("(gmx_[a-z0-9_]+)"\)', text))
    for name in NEW:
        declaration(name)
        assert hasattr(lib, name), name
        assert name in guarded and re.search(r"\b" + name + r"\([^)]*\)\s*try\s*\{", text), name


def test_ctypes_signatures_match_the_header():
    for name in NEW:
        ret, params = declaration(name)
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is CTYPE[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for p, a in zip(params, argtypes):
            assert a is CTYPE[p], (name, p, a)


def test_the_left_out_bits_of_the_header():
    text = open(os.path.join(ROOT, "include", "gmx.h")).read()
    for k, v in {"LEFT_OUT_FORWARD": "0x40", "LEFT_OUT_REVERSE": "0x80"}.items():
        assert re.search(r"#define GMX_OUTCOME_" + k + r"\s+" + v + r"\b", text), k
    assert "bits 6-7  zero" not in text


def test_null_handles_are_errors_not_crashes():
    lib = _lib.load()
    assert lib.gmx_engine_set_max_candidates(None, 1) == -1 and b"null engine" in lib.gmx_last_error()
    assert lib.gmx_engine_max_candidates(None) == 0
    assert lib.gmx_group_set_max_candidates(None, 1) == -1 and b"null group" in lib.gmx_last_error()


def test_python_wrappers():
    assert callable(Quasimapper.set_max_candidates) and callable(QuasimapperGroup.set_max_candidates)
    assert isinstance(Quasimapper.max_candidates, property)


def test_gram_genotype_help_lists_the_flag_as_an_engine_extension():
    from ingest_formats_common import gram
    r = gram("genotype", "--help")
    m = re.search(r"--max_candidates arg(.*?)(?:\n  --|\Z)", r.stdout, flags=re.S)
    assert m and "engine extension" in m.group(1) and "read_filter.json" in m.group(1), r.stdout


@pytest.mark.parametrize("value", [["0"], ["x"], ["-1"], ["1.5"], ["4294967296"], [""], []], ids=lambda v: "none" if not v else repr(v[0]))
def test_gram_refuses_a_bad_value_before_it_creates_an_engine(tmp_path, value):
    """Exit 1 with a message, nothing written: the gram_dir does not even exist."""
    from ingest_formats_common import gram
    out = tmp_path / "g"
    r = gram("genotype", "--gram_dir", str(tmp_path / "absent"), "--reads", str(tmp_path / "absent.fq"), "--sample_id", "s", "--ploidy", "diploid",
             "--kmer_size", "6", "--genotype_dir", str(out), "--seed", "1", "--max_candidates", *value)
    assert r.returncode == 1, r.stdout
    assert "max_candidates" in r.stdout and not out.exists(), r.stdout

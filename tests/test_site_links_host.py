"""Links between nearby sites (gmx_engine_record_links), what needs no GPU: the layout of the link block against its
formula, the refusals of gmx_index_link_layout and of `gram genotype --site_links`, the declarations, and that the test case holds
what the GPU tests (test_site_links.py) rely on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gramtools_amd import Index, Quasimapper, QuasimapperGroup, _lib, link_matrix
from gramtools_amd.synth import bracket_to_ints
import site_links_common as slc
from test_read_outcomes_host import declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gramtools_amd", "csrc")
GMX_EINVAL = -1
NEW = ("gmx_index_link_layout", "gmx_engine_record_links", "gmx_engine_links", "gmx_coverage_fetch_links", "gmx_group_record_links")
CTYPE = {"int": C.c_int, "gmx_engine *": C.c_void_p, "gmx_group *": C.c_void_p, "gmx_index *": C.c_void_p,  # (declaration() drops the const)
         "uint32_t *": C.POINTER(C.c_uint32), "uint64_t *": C.POINTER(C.c_uint64), "uint64_t": C.c_uint64}

ALLELES = [2, 3, 4, 2, 9, 3, 2, 4, 8, 2, 3, 2]  # 2-4-allele sites, a 9-allele site, an 8-allele one, sites in the last positions


def flat_prg(alleles=ALLELES, seed=3):
    """Random bases with one site of alleles[i] distinct two-base alleles every 7 bases."""
    rng = np.random.default_rng(seed)
    two = [(a, b) for a in range(1, 5) for b in range(1, 5)]
    prg, m = [], 5
    for n in alleles:
        prg += [int(x) for x in rng.integers(1, 5, size=7)] + [m]
        for i in rng.permutation(16)[:n]:
            prg += [two[i][0], two[i][1], m + 1]
        m += 2
    prg += [int(x) for x in rng.integers(1, 5, size=7)]
    return np.asarray(prg, dtype=np.uint32)


@pytest.fixture(scope="module")
def flat_ix():
    return Index(flat_prg(), 4)


@pytest.fixture(scope="module")
def nested_ix():
    return Index(bracket_to_ints("acgtacgtta[ac,t[g,c]a]ttgacca[a,g]ccatgca"), 4)


@pytest.mark.parametrize("span", [1, 3, 7])
def test_the_layout_is_the_formula(flat_ix, span):
    assert flat_ix.n_alleles.tolist() == ALLELES
    off = flat_ix.link_layout(span)
    assert off.dtype == np.uint64 and off.tolist() == slc.layout(ALLELES, span).tolist()
    a = [x if x <= 8 else 0 for x in ALLELES] + [0] * 8
    assert [int(off[s + 1] - off[s]) for s in range(len(ALLELES))] == [a[s] * sum(a[s + 1:s + 1 + span]) for s in range(len(ALLELES))]
    assert off[0] == 0 and off[4] == off[5] and off[-1] == off[-2]  # the 9-allele site and the last site own no word
    if span == 7:  # a site in the last `span` positions: its block stops at the last site
        assert int(off[9] - off[8]) == 8 * (2 + 3 + 2)
    # link_matrix cuts M(s, d) where the formula puts it
    words = np.arange(int(off[-1]), dtype=np.uint32)
    for s, d in [(0, 1), (1, 2), (2, 3), (3, 2), (8, 3)]:
        m = link_matrix(flat_ix.n_alleles, off, words, s, d)
        if d > span or a[s + d] == 0:
            assert m.size == 0
        else:
            at = slc.matrix_start(ALLELES, off, s, d)
            assert m.shape == (a[s], a[s + d]) and m.reshape(-1).tolist() == list(range(at, at + m.size))
    assert link_matrix(flat_ix.n_alleles, off, words, 4, 1).size == 0 and link_matrix(flat_ix.n_alleles, off, words, 3, 1).size == 0


def test_span_zero_owns_no_word(flat_ix):
    assert not flat_ix.link_layout(0).any()


def test_the_layout_refuses_a_nested_index_and_a_bad_span(flat_ix, nested_ix):
    lib = flat_ix.lib
    assert nested_ix.is_nested
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.gmx_index_link_layout(nested_ix.h, 3, p, nested_ix.n_sites + 1) == GMX_EINVAL and b"flat" in lib.gmx_last_error()
    for span in (-1, 8):
        assert lib.gmx_index_link_layout(flat_ix.h, span, p, flat_ix.n_sites + 1) == GMX_EINVAL and b"span" in lib.gmx_last_error()
    assert lib.gmx_index_link_layout(flat_ix.h, 3, p, flat_ix.n_sites) == GMX_EINVAL and b"n_sites_plus_1" in lib.gmx_last_error()
    assert lib.gmx_index_link_layout(None, 3, p, 1) == GMX_EINVAL
    assert lib.gmx_index_link_layout(flat_ix.h, 3, None, flat_ix.n_sites + 1) == GMX_EINVAL


@pytest.mark.parametrize("value", [["0"], ["8"], ["x"], ["-1"], ["12"], [""], []], ids=lambda v: "none" if not v else repr(v[0]))
def test_gram_refuses_a_bad_span_before_it_creates_an_engine(tmp_path, value):
    """Exit 1 with a message, nothing written: the gram_dir does not even exist."""
    from ingest_formats_common import gram
    out = tmp_path / "g"
    r = gram("genotype", "--gram_dir", str(tmp_path / "absent"), "--reads", str(tmp_path / "absent.fq"), "--sample_id", "s", "--ploidy", "diploid",
             "--kmer_size", "6", "--genotype_dir", str(out), "--seed", "1", "--site_links", *value)
    assert r.returncode == 1, r.stdout
    assert "site_links" in r.stdout and not out.exists(), r.stdout


def test_gram_genotype_help_lists_the_flag():
    from ingest_formats_common import gram
    r = gram("genotype", "--help")
    m = re.search(r"--site_links arg(.*?)(?:\n  --|\Z)", r.stdout, flags=re.S)
    assert m and "engine extension" in m.group(1) and "coverage/site_links.json" in m.group(1), r.stdout


def test_the_entry_points_are_declared_exported_and_guarded():
    lib = C.CDLL(_lib.LIB) if os.path.exists(_lib.LIB) else _lib.load()
    text = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".cpp")))
    guarded = set(re.findall(r'GMX_GUARD_(?:INT|VOID|PTR|ZERO)\("(gmx_[a-z0-9_]+)"\)', text))
    for name in NEW:
        ret, params = declaration(name)
        assert hasattr(lib, name), name
        assert name in guarded and re.search(r"\b" + name + r"\([^)]*\)\s*try\s*\{", text), name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is CTYPE[ret], (name, ret, restype)
        assert [CTYPE[p] for p in params] == list(argtypes), (name, params, argtypes)


def test_null_handles_are_errors_not_crashes():
    lib = _lib.load()
    assert lib.gmx_engine_record_links(None, 3) == GMX_EINVAL and b"null engine" in lib.gmx_last_error()
    assert lib.gmx_engine_links(None) == 0
    assert lib.gmx_coverage_fetch_links(None, None, 0) == GMX_EINVAL
    assert lib.gmx_group_record_links(None, 3) == GMX_EINVAL and b"null group" in lib.gmx_last_error()
    for cls in (Quasimapper, QuasimapperGroup):
        assert callable(cls.record_links) and callable(cls.links)


def test_the_case_holds_what_the_gpu_tests_rely_on():
    """A counted pair at every distance 1..3, a pair whose left locus is the allele the read starts inside, a pair skipped at the
    wide site beside pairs that count, multi-instance tasks over two sites or more, a row with two non-zero cells; and
    locus_finder's allele ids are the columns of allele_sum_coverage."""
    prg, k, reads, _ = slc.case()
    assert 1500 <= prg.size <= 4000 and k in (5, 6) and len(reads) <= 1000 and all(40 <= len(r) <= 80 for r in reads)
    tasks = slc.check_case_contents()
    crossed = [len(loci) for _, n, loci, _ in tasks if n == 1]
    assert sum(1 for c in crossed if 3 <= c <= 6) > len(crossed) // 2
    ix = Index(prg, k)
    assert ix.n_alleles.tolist() == slc.oracle_alleles().tolist() and ix.uses_grouped_log and not ix.is_nested
    for span in (1, 3, 7):
        off, words = slc.expectation(span)
        assert ix.link_layout(span).tolist() == off.tolist() and words.any()
    # span 1 and span 3 hold the same d = 1 matrices
    one, three = slc.expectation(1), slc.expectation(3)
    for s in range(ix.n_sites - 1):
        assert (link_matrix(ix.n_alleles, one[0], one[1], s, 1) == link_matrix(ix.n_alleles, three[0], three[1], s, 1)).all()


def test_the_shared_routine_on_the_host_under_sanitizers(tmp_path):
    """gmx_link_path and gmx_link_offsets as the host compiles them (tests/link_path/link_path_check.cpp, a stand-alone program):
    pairs seven apart, non-linkable sites in the middle, alleles of 15 and more, the batch's edge at four loci, the allele the read
    starts inside — built with -fsanitize=address,undefined."""
    import subprocess
    exe = tmp_path / "link_path_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           "-o", str(exe), os.path.join(ROOT, "tests", "link_path", "link_path_check.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout

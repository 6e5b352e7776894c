"""Coverage per strand, the parts that need no GPU: the entry points are declared in include/gmx.h, exported by the library,
closed by a GMX_GUARD_* function-try-block and mirrored with the header's signatures in gramtools_amd/_lib.py; null handles
are errors; the help text lists the flag."""
import ctypes as C
import os
import re

from gramtools_amd import _lib, Quasimapper, QuasimapperGroup
from test_read_outcomes_host import declaration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gramtools_amd", "csrc")
NEW = ("gmx_engine_record_strands", "gmx_coverage_fetch_strand", "gmx_group_record_strands")
CTYPE = {"int": C.c_int, "gmx_engine *": C.c_void_p, "gmx_group *": C.c_void_p, "uint32_t *": C.POINTER(C.c_uint32)}


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


def test_null_handles_are_errors_not_crashes():
    lib = _lib.load()
    assert lib.gmx_engine_record_strands(None, 1) == -1 and b"null engine" in lib.gmx_last_error()
    assert lib.gmx_coverage_fetch_strand(None, 0, None, None, None) == -1
    assert lib.gmx_group_record_strands(None, 1) == -1 and b"null group" in lib.gmx_last_error()


def test_python_wrappers():
    import inspect
    assert callable(Quasimapper.record_strands) and callable(QuasimapperGroup.record_strands)
    assert inspect.signature(Quasimapper.coverage).parameters["strand"].default is None
    assert list(inspect.signature(QuasimapperGroup.coverage).parameters)[1:] == ["member", "strand"]


def test_gram_genotype_help_lists_the_flag():
    from ingest_formats_common import gram
    r = gram("genotype", "--help")
    assert "--strand_coverage" in r.stdout, r.stdout
    for f in ("allele_sum_coverage.forward", "allele_base_coverage.forward.json"):
        assert f in r.stdout, f


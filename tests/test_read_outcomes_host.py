"""Per-read mapping outcomes, the parts that need no GPU: the three entry points are declared in include/gmx.h, exported by
the library, closed by a GMX_GUARD_* function-try-block and mirrored with the header's signatures in gramtools_amd/_lib.py."""
import ctypes as C
import os
import re

from gramtools_amd import _lib, Quasimapper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmx_engine_record_outcomes", "gmx_engine_outcome_count", "gmx_engine_fetch_outcomes", "gmx_group_outcome_count",
       "gmx_group_fetch_outcomes")
CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "gmx_engine *": C.c_void_p, "gmx_group *": C.c_void_p, "uint8_t *": C.POINTER(C.c_uint8)}


def header_text():
    text = open(os.path.join(ROOT, "include", "gmx.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def declaration(name):
    """(return type, [parameter types]) of `name` as include/gmx.h declares it."""
    m = re.search(r"^\s*([a-z0-9_]+ \*?)\s*" + name + r"\(([^)]*)\);", header_text(), flags=re.M)
    assert m, name + " is not declared in include/gmx.h"
    params = []
    for p in m.group(2).split(","):
        t = re.match(r"\s*(?:const\s+)?([a-z0-9_]+)\s*(\*?)\s*[a-z_0-9]+\s*$", p)
        assert t, p
        params.append(t.group(1) + (" *" if t.group(2) else ""))
    return m.group(1).strip(), params


def test_the_entry_points_are_declared_and_exported():
    lib = C.CDLL(_lib.LIB) if os.path.exists(_lib.LIB) else _lib.load()
    for name in NEW:
        declaration(name)
        assert hasattr(lib, name), name


def test_the_entry_points_are_guarded():
    csrc = os.path.join(ROOT, "gramtools_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp")))
    guarded = set(re.findall(r'GMX_GUARD_(?:INT|VOID|PTR|ZERO)\("(gmx_[a-z0-9_]+)"\)', text))
    assert set(NEW) <= guarded, set(NEW) - guarded
    for name in NEW:  # the guard closes the function's own try block
        assert re.search(r"\b" + name + r"\([^)]*\)\s*try\s*\{", text), name


def test_ctypes_signatures_match_the_header():
    for name in NEW:
        ret, params = declaration(name)
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is CTYPE[ret], (name, ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for p, a in zip(params, argtypes):
            assert a is CTYPE[p] or (p.endswith("*") and a is C.c_void_p), (name, p, a)


def test_outcome_codes_of_the_header():
    text = open(os.path.join(ROOT, "include", "gmx.h")).read()
    want = {"SKIPPED": "0", "MISSING_KMER": "1", "NO_EXTENSION": "2", "MAPPED": "3", "MULTI_FORWARD": "0x10", "MULTI_REVERSE": "0x20"}
    for k, v in want.items():
        assert re.search(r"#define GMX_OUTCOME_" + k + r"\s+" + v + r"\b", text), k


def test_null_engine_is_an_error_not_a_crash():
    lib = _lib.load()
    assert lib.gmx_engine_record_outcomes(None, 1) == -1
    assert lib.gmx_engine_outcome_count(None) == -1 and b"null engine" in lib.gmx_last_error()
    assert lib.gmx_group_outcome_count(None) == -1 and lib.gmx_group_fetch_outcomes(None, 0, 0, None) == -1
    out = (C.c_uint8 * 4)()
    assert lib.gmx_engine_fetch_outcomes(None, 0, 4, out) == -1


def test_python_wrapper_has_the_methods():
    for m in ("record_outcomes", "outcome_count", "outcomes"):
        assert callable(getattr(Quasimapper, m))


def test_gram_genotype_help_lists_the_flag():
    from ingest_formats_common import gram
    r = gram("genotype", "--help")
    assert "--read_outcomes" in r.stdout and "read_outcomes.bin" in r.stdout, r.stdout
    text = open(os.path.join(ROOT, "gramtools_amd", "csrc", "gram_main.cpp")).read()
    m = re.search(r"const char \*kGenotypeHelp =(.*?);\n", text, flags=re.S)
    assert m and "--read_outcomes" in m.group(1)


def parse_outcomes_file(data: bytes):
    """read_outcomes.bin: "GMXO", uint32 version 1, uint64 read count (little-endian), then one byte per read."""
    import struct
    if len(data) < 16:
        raise ValueError("shorter than its header")
    magic, version, n = struct.unpack_from("<4sIQ", data, 0)
    if magic != b"GMXO" or version != 1 or len(data) != 16 + n:
        raise ValueError(f"not a read_outcomes.bin: {magic!r}, version {version}, {n} reads in {len(data)} bytes")
    return bytes(data[16:])


def test_read_outcomes_header_is_the_one_gram_writes():
    """The helper on a file made by hand, and on the bytes gram_main.cpp writes in front of the reads' bytes."""
    import struct
    import pytest
    body = bytes([0x0F, 0x07, 0x1D, 0x00, 0x2B])
    assert parse_outcomes_file(b"GMXO" + struct.pack("<IQ", 1, 5) + body) == body
    assert parse_outcomes_file(b"GMXO" + struct.pack("<IQ", 1, 0)) == b""
    for bad in (b"GMXO" + struct.pack("<IQ", 2, 5) + body, b"GMXX" + struct.pack("<IQ", 1, 5) + body, b"GMXO" + struct.pack("<IQ", 1, 6) + body, b"GMXO"):
        with pytest.raises(ValueError):
            parse_outcomes_file(bad)
    text = open(os.path.join(ROOT, "gramtools_amd", "csrc", "gram_main.cpp")).read()
    assert "header[16] = {'G', 'M', 'X', 'O', 1, 0, 0, 0}" in text and "header[8 + i] = (unsigned char)((total_reads >> (8 * i)) & 0xFF)" in text

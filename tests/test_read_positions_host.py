"""Per-read positions, the parts that need no GPU: the six entry points are declared in include/gmx.h, exported by the library,
closed by a GMX_GUARD_* function-try-block and mirrored with the header's signatures in gramtools_amd/_lib.py; the host build of
the device headers (tests/hostemu) still compiles and maps as before; the file header `gram` writes parses."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from gramtools_amd import _lib, Quasimapper, QuasimapperGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gmx_engine_record_positions", "gmx_engine_position_count", "gmx_engine_fetch_positions", "gmx_group_record_positions",
       "gmx_group_position_count", "gmx_group_fetch_positions")
CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "gmx_engine *": C.c_void_p, "gmx_group *": C.c_void_p,
         "uint32_t *": C.POINTER(C.c_uint32)}


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
    # (the version script hides the library's operator new / delete only: nothing in it may name the new functions as local)
    assert not set(NEW) & set(re.findall(r"gmx_[a-z0-9_]+", open(os.path.join(ROOT, "gramtools_amd", "csrc", "libgmx.map")).read()))


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


def test_null_handles_are_errors_not_crashes():
    lib = _lib.load()
    assert lib.gmx_engine_record_positions(None, 1) == -1
    assert lib.gmx_engine_position_count(None) == -1 and b"null engine" in lib.gmx_last_error()
    assert lib.gmx_group_record_positions(None, 1) == -1 and b"null group" in lib.gmx_last_error()
    assert lib.gmx_group_position_count(None) == -1 and lib.gmx_group_fetch_positions(None, 0, 0, None) == -1
    out = (C.c_uint32 * 16)()
    assert lib.gmx_engine_fetch_positions(None, 0, 4, out) == -1


def test_python_wrappers_have_the_methods():
    for cls in (Quasimapper, QuasimapperGroup):
        for m in ("record_positions", "position_count", "positions"):
            assert callable(getattr(cls, m)), (cls, m)


def test_gram_genotype_help_lists_the_flag():
    from ingest_formats_common import gram
    r = gram("genotype", "--help")
    assert "--read_positions" in r.stdout and "read_positions.bin" in r.stdout and "read_positions.json" in r.stdout, r.stdout


def parse_positions_file(data: bytes):
    """read_positions.bin: "GMXP", uint32 version 1, uint64 read count (little-endian), then four uint32 per read."""
    if len(data) < 16:
        raise ValueError("shorter than its header")
    magic, version, n = struct.unpack_from("<4sIQ", data, 0)
    if magic != b"GMXP" or version != 1 or len(data) != 16 + 16 * n:
        raise ValueError(f"not a read_positions.bin: {magic!r}, version {version}, {n} reads in {len(data)} bytes")
    return np.frombuffer(data, dtype="<u4", offset=16).reshape(n, 4)


def test_read_positions_header_is_the_one_gram_writes():
    """The helper on files made by hand, and on the bytes gram_main.cpp writes in front of the records."""
    body = np.asarray([[17, 1, 0, 0], [0, 0, 2040, 10], [5, 0xFFFFFFFF, 5, 2]], dtype="<u4")
    assert parse_positions_file(b"GMXP" + struct.pack("<IQ", 1, 3) + body.tobytes()).tolist() == body.tolist()
    assert parse_positions_file(b"GMXP" + struct.pack("<IQ", 1, 0)).shape == (0, 4)
    for bad in (b"GMXP" + struct.pack("<IQ", 2, 3) + body.tobytes(), b"GMXO" + struct.pack("<IQ", 1, 3) + body.tobytes(),
                b"GMXP" + struct.pack("<IQ", 1, 4) + body.tobytes(), b"GMXP" + struct.pack("<IQ", 1, 3) + body.tobytes()[:-1], b"GMXP"):
        with pytest.raises(ValueError):
            parse_positions_file(bad)
    text = open(os.path.join(ROOT, "gramtools_amd", "csrc", "gram_main.cpp")).read()
    assert "header[16] = {'G', 'M', 'X', 'P', 1, 0, 0, 0}" in text


def test_the_host_build_of_the_device_headers_is_unchanged_and_maps_as_before():
    """tests/hostemu/hostemu.cpp calls gmx_cover_task with seven arguments and is not touched: it compiles against the headers as
    they are now, and a repeat with classes and non-variant instances gives the oracle's coverage through it."""
    from common import hostemu_map, oracle_map
    from gramtools_amd import master_seeds
    from test_many_instances import tandem_prg, tandem_reads
    src = open(os.path.join(ROOT, "tests", "hostemu", "hostemu.cpp")).read()
    calls = re.findall(r"gmx_cover_task\(([^;]*)\);", src)
    assert len(calls) >= 3 and all(len(c.split(",")) == 7 for c in calls), calls
    prg, unit, site_at, alt = tandem_prg(12, 60, 3)
    reads = tandem_reads(unit, site_at, alt, 50, 4)
    seeds = master_seeds(9, [len(reads)])
    got, _, rc = hostemu_map(prg, 8, reads, seeds)
    assert rc == 0 and got == oracle_map(prg, 8, reads, seeds)

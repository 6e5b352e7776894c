"""Plain gzip FASTQ decoded on the device (include/gmx.h gmx_ingest_submit_gzip, gmx_ingest.hip gmx_gz_*_kernel):
one deflate stream per member cut into pieces decoded side by side from speculative block starts, repaired on the device where
they do not line up, CRC-32 / ISIZE checked per member. Checked against zlib (the text), the host packer (the reads) and, through
`gram`, against the host reader and the plain text."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from test_ingest import check_reads, fastq, _gram, _cli_fastq

pytestmark = pytest.mark.gpu

GZ_HDR = b"\x1f\x8b\x08\x00\0\0\0\0\0\xff"
GZ_UNREPAIRED, GZ_LOOKAHEAD, GZ_PIECE_BOUND, GZ_MEMBER_ENDS, GZ_TEXT_LIMIT = 16, 32, 64, 128, 256


def member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, header=GZ_HDR, crc=None, isize=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    body = c.compress(data) + c.flush()
    crc = zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc
    isize = len(data) & 0xFFFFFFFF if isize is None else isize
    return header + body + struct.pack("<II", crc, isize)


def decode(data: bytes, chunk=None, look=1 << 18, max_text=8 << 20, cuts=None, allow=0):
    """The file through one Ingest in chunks (of `chunk` bytes, or cut at `cuts`) with `look` bytes of look-ahead: (text of
    the whole file as the chunks hand it over, the results, the ingest). allow: status bits that do not end it (text that is
    no FASTQ: the record scan's)."""
    from gramtools_amd import Ingest
    ing = Ingest(max_text_bytes=max_text)
    n = len(data)
    if cuts is None:
        chunk = chunk or max(n, 1)
        cuts = list(range(chunk, n, chunk))
    bounds = [0] + [c for c in cuts if 0 < c < n] + [n]
    text, results, tail = b"", [], 0
    for k in range(len(bounds) - 1):
        c0, c1 = bounds[k], bounds[k + 1]
        final = c1 == n
        ing.submit_gzip(k % 2, data[c0:c1 if final else min(n, c1 + look)], c1 - c0, final)
        res = ing.wait(k % 2)
        results.append(res)
        if res.status & ~allow:
            return None, results, ing
        t = ing.fetch_text(k % 2)
        text += t[tail:]
        tail = int(res.tail_bytes)
    return text, results, ing


@pytest.fixture
def pieces(monkeypatch):
    def set_(n):
        monkeypatch.setenv("GMX_GZ_PIECE", str(n))
    return set_


@pytest.mark.parametrize("level,strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                                            (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FILTERED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE),
                                            (6, zlib.Z_FIXED)])
@pytest.mark.parametrize("piece,chunk", [(1024, None), (4096, 150001), (65536, 77777)])
def test_text_equals_zlib(pieces, level, strategy, piece, chunk):
    pieces(piece)
    rng = np.random.default_rng(level * 31 + strategy * 7 + piece)
    text, _ = fastq(rng, 2500, 100, 150)
    data = member(text, level, strategy)
    got, res, ing = decode(data, chunk=chunk)
    assert res[-1].status == 0 and all(r.status == 0 for r in res), [r.status for r in res]
    assert got == text
    ing.close()


@pytest.mark.parametrize("cuts", [[1], [9], [10], [11], [2000, 2001, 2002], [5000, 5003, 40000, 40001]])
def test_chunk_cuts_at_every_kind_of_boundary(pieces, cuts):
    """Chunks of one byte, cuts inside the header, a block, a record; the stream position and window travel between them."""
    pieces(2048)
    rng = np.random.default_rng(sum(cuts))
    text, _ = fastq(rng, 800, 80, 150)
    data = member(text, 6)
    got, res, ing = decode(data, cuts=cuts)
    assert all(r.status == 0 for r in res), [r.status for r in res]
    assert got == text
    ing.close()


@pytest.mark.parametrize("crlf,lower,bad_every,lo,hi", [(False, False, 0, 150, 150), (True, False, 7, 1, 300), (False, True, 3, 20, 90)])
def test_reads_equal_the_host_packer(pieces, crlf, lower, bad_every, lo, hi):
    pieces(4096)
    rng = np.random.default_rng(lo + hi)
    text, seqs = fastq(rng, 3000, lo, hi, bad_every=bad_every, crlf=crlf, lower=lower)
    from gramtools_amd import Ingest
    ing = Ingest(max_text_bytes=8 << 20)
    ing.submit_gzip(0, member(text, 6), len(member(text, 6)), True)
    res = ing.wait(0)
    assert ing.fetch_text(0) == text
    check_reads(ing, 0, res, seqs)
    ing.close()


def test_members(pieces):
    pieces(2048)
    rng = np.random.default_rng(5)
    ta, _ = fastq(rng, 400, 100, 150)
    tb, _ = fastq(rng, 700, 50, 150)
    tc, _ = fastq(rng, 3, 50, 60)
    a, b = member(ta), member(tb, 1)
    fields = b"\x1f\x8b\x08\x1e\0\0\0\0\0\x03" + struct.pack("<H", 5) + b"AB\x01\x00Z" + b"name.fq\0" + b"a comment\0" + b"\x12\x34"
    c = member(tc, 9, header=fields)  # FEXTRA + FNAME + FCOMMENT + FHCRC
    cat = a + b + c + member(tc)      # (the last two: member ends inside one piece)
    whole = ta + tb + tc + tc
    got, res, ing = decode(cat)
    assert all(r.status == 0 for r in res) and got == whole
    got, res, ing = decode(cat, cuts=[len(a), len(a) + len(b)])  # member ends exactly at chunk boundaries
    assert all(r.status == 0 for r in res) and got == whole
    got, res, ing = decode(cat + b"\0" * 1000, cuts=[len(cat) + 10])  # trailing zeros, one chunk of zeros only
    assert all(r.status == 0 for r in res) and got == whole
    got, res, ing = decode(gzip.compress(b""))  # a header and an empty member
    assert res[0].status == 0 and got == b"" and res[0].n_reads == 0
    ing.close()


def test_many_tiny_members_in_a_piece(pieces):
    pieces(4096)
    rng = np.random.default_rng(8)
    text, _ = fastq(rng, 200, 30, 40)
    recs = text.split(b"\n@")
    parts = [recs[0]] + [b"@" + r for r in recs[1:]]
    parts = [p + b"\n" for p in parts[:-1]] + [parts[-1]]
    data = b"".join(member(p) for p in parts)
    _, res, ing = decode(data)
    assert res[-1].status & GZ_MEMBER_ENDS  # (members of ~100 bytes: far more than a piece records)
    ing.close()


def test_repairs(pieces, monkeypatch):
    """Test hook: the finder takes a later block start for every 3rd piece and none for every 4th; the link kernel decodes them
    again from where the piece before ended. The text is unchanged, the status 0, and the repairs are counted."""
    pieces(8192)
    monkeypatch.setenv("GMX_GZ_TEST_FIND", "3,4")
    rng = np.random.default_rng(9)
    text, _ = fastq(rng, 6000, 150, 150)
    data = member(text, 6)
    got, res, ing = decode(data, chunk=400000)
    assert all(r.status == 0 for r in res) and got == text
    assert ing.gzip_repairs() > 0
    ing.close()


def test_damage_is_reported(pieces):
    pieces(4096)
    rng = np.random.default_rng(10)
    text, _ = fastq(rng, 2000, 150, 150)
    good = member(text, 6)
    cases = {
        "truncated": good[:-5000],
        "flipped": good[:len(good) // 2] + bytes(x ^ 0x5A for x in good[len(good) // 2:len(good) // 2 + 40]) + good[len(good) // 2 + 40:],
        "crc": member(text, 6, crc=(zlib.crc32(text) ^ 1) & 0xFFFFFFFF),
        "isize": member(text, 6, isize=len(text) + 1),
        "tail garbage": good + b"\x01\x02\x03",
    }
    for name, data in cases.items():
        _, res, ing = decode(data)
        assert res[-1].status != 0, name
        assert res[-1].status != 0 and not (res[-1].status == 0 and res[-1].n_reads), name
        ing.close()
    _, res, ing = decode(good, chunk=len(good) // 2, look=0)  # no look-ahead: the chunk's last block cannot finish
    assert res[0].status & GZ_LOOKAHEAD
    ing.close()
    bomb = member(b"A" * (24 << 20), 9)  # 1000:1: passes the piece bound
    _, res, ing = decode(bomb, max_text=64 << 20)
    assert res[0].status & GZ_PIECE_BOUND
    ing.close()


def test_text_larger_than_the_ingest(pieces):
    pieces(65536)
    data = member(b"@r\nACGT\n+\nIIII\n" * 20000, 6)  # 300 KB of text
    _, res, ing = decode(data, max_text=1 << 16)
    assert res[0].status & (GZ_TEXT_LIMIT | GZ_PIECE_BOUND)
    ing.close()


def test_allocation_failure_then_reset(pieces):
    from gramtools_amd import Ingest, _lib, GmxError
    pieces(4096)
    lib = _lib.load()
    rng = np.random.default_rng(11)
    text, _ = fastq(rng, 300, 150, 150)
    data = member(text)
    ing = Ingest(max_text_bytes=4 << 20)
    failed = 0
    try:
        for n in range(1, 20):
            lib.gmx_debug_fail_alloc(n)
            try:
                ing.submit_gzip(0, data, len(data), True)
            except GmxError as e:
                assert e.code == -6  # GMX_ENOMEM
                failed += 1
                ing.reset()
                continue
            finally:
                lib.gmx_debug_fail_alloc(0)
            break
    finally:
        lib.gmx_debug_fail_alloc(0)
    assert failed >= 1
    res = ing.wait(0)
    assert res.status == 0 and ing.fetch_text(0) == text
    ing.reset()
    ing.submit_gzip(1, data, len(data), True)
    res = ing.wait(1)
    assert res.status == 0 and ing.fetch_text(1) == text
    ing.close()


# ---- through the `gram` executable ------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,crlf", [(None, False), ("3000", False), ("7777", True)])
def test_gram_parse_check_device_line_plain_gzip(tmp_path, chunk, crlf):
    """`gram _parse_check` (GMX_PARSE_CHECK_DEVICE=1) on a plain .gz: the device line hashes to what the host parsers make of it
    (until this route existed it read `device declined`)."""
    text = _cli_fastq(4000, 22, crlf=crlf).encode()
    path = tmp_path / "r.fastq.gz"
    path.write_bytes(gzip.compress(text, 6) + gzip.compress(text[:0]))
    env = {"GMX_PARSE_CHECK_DEVICE": "1", "GMX_GZ_PIECE": "2048"}
    if chunk:
        env["GMX_GZ_CHUNK"] = chunk
    out = _gram("_parse_check", str(path), "1", env=env)
    assert out.returncode == 0, out.stdout
    lines = [l for l in out.stdout.strip().splitlines() if l.split()[0] in ("fast", "slow", "device")]
    assert len(lines) == 3 and lines[0].startswith("fast ") and lines[2].startswith("device "), out.stdout
    assert lines[0][5:] == lines[1][5:] == lines[2][7:], out.stdout


def _genotype_outputs(tmp_path, name, files, env, extra=()):
    import json
    out = tmp_path / name
    r = _gram("genotype", "--gram_dir", str(tmp_path), "--reads", *[str(tmp_path / f) for f in files], "--sample_id", "s", "--ploidy", "diploid",
              "--kmer_size", "6", "--genotype_dir", str(out), "--seed", "1234", "--max_threads", "1", *extra, env=env)
    if r.returncode != 0:
        return r, None
    counters = [l for l in r.stdout.splitlines() if l.startswith("Count ")]
    geno = sorted(p.relative_to(out).as_posix() for p in out.rglob("*") if p.is_file())
    return r, ([(out / "coverage" / f).read_bytes() for f in ("allele_sum_coverage", "allele_base_coverage.json", "grouped_allele_counts_coverage.json")],
               counters, json.loads((out / "read_stats.json").read_text()), geno)


def test_gram_genotype_plain_gzip_on_the_device(tmp_path):
    """`gram genotype --max_threads 1` on a plain .fastq.gz (device route) and a BGZF one: coverage files, read_stats.json, the
    genotype outputs' names and the counters equal those of the plain FASTQ, of GMX_HOST_GZ=1, of --devices 0,0 (host path) and
    of the host reader taking over at chunk 0 and at a later chunk. A damaged file still fails."""
    from test_ingest import bgzf
    from gramtools_amd.synth import random_ref, snp_prg, simulate_snp_reads
    ref = random_ref(3000, 4)
    prg, pos, alts, n_alts = snp_prg(ref, 40, 5, multi_allelic_frac=0.3)
    (tmp_path / "prg").write_bytes(np.array(prg, dtype="<u4").tobytes())
    reads = simulate_snp_reads(ref, pos, alts, n_alts, 7300, 60, 6)
    txt = ["".join("ACGT"[b - 1] for b in r) for r in reads]
    txt[17] = txt[17][:10] + "N" + txt[17][11:]
    fq = lambda rs: "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(rs)).encode()  # noqa: E731
    a, b = fq(txt[:5100]), fq(txt[5100:])
    (tmp_path / "a.fq").write_bytes(a)
    (tmp_path / "b.fq").write_bytes(b)
    (tmp_path / "a.fq.gz").write_bytes(gzip.compress(a, 6))
    (tmp_path / "b.fq.gz").write_bytes(bgzf(b, block=9000))
    small = {"GMX_GZ_CHUNK": "20000", "GMX_GZ_PIECE": "4096", "GMX_FEED_TRACE": "1"}
    runs = (("plain", ("a.fq", "b.fq"), {}, ()), ("device", ("a.fq.gz", "b.fq.gz"), dict(small), ()),
            ("host", ("a.fq.gz", "b.fq.gz"), {"GMX_HOST_GZ": "1"}, ()),
            ("two-engines", ("a.fq.gz", "b.fq.gz"), dict(small), ("--devices", "0,0")),
            ("fail-0", ("a.fq.gz", "b.fq"), dict(small, GMX_INGEST_TEST_FAIL_CHUNK="0"), ()),
            ("fail-2", ("a.fq.gz", "b.fq"), dict(small, GMX_GZ_CHUNK="3000", GMX_INGEST_TEST_FAIL_CHUNK="2", GMX_FASTQ_BLOCK="200000"), ()))
    outs = {}
    for name, files, env, extra in runs:
        r, outs[name] = _genotype_outputs(tmp_path, name, files, env, extra)
        assert outs[name] is not None, r.stdout
        if name in ("device", "fail-2"):  # (the route really taken: the feed's trace names its chunks)
            assert "gzip chunk decoded" in r.stdout, r.stdout
        if name == "two-engines":
            assert "gzip chunk" not in r.stdout, r.stdout
        if name.startswith("fail-"):
            assert "gzip decoder gave up" in r.stdout, r.stdout
    for name in ("device", "host", "two-engines", "fail-0", "fail-2"):
        assert outs[name][:3] == outs["plain"][:3], name
        assert outs[name][3] == outs["plain"][3], name
    d = bytearray(gzip.compress(a, 6))
    d[len(d) // 2] ^= 0x55
    (tmp_path / "bad.fq.gz").write_bytes(bytes(d))
    r, res = _genotype_outputs(tmp_path, "bad", ("bad.fq.gz",), dict(small))
    assert r.returncode == 1, r.stdout

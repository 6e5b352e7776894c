"""Shared by test_record_scan_scale.py (GPU) and test_record_scan_scale_host.py (no GPU): reads files large enough to reach the
scale edges of the device record scan (gmx_ingest_records.h), generated with numpy and no Python loop per read; the arithmetic
of the ingest's tables (gmx_ingest_create) restated; the plain-Python parse the device is compared with; the capacity cases and
the hand-built texts of the edge sweep. Nothing here touches the code under test."""
from collections import namedtuple

import numpy as np

from ingest_formats_common import parse as parse_seq

CARRY = 1 << 20     # ING_CARRY_MAX: the chunk's own text starts at this offset of the slot's buffer, the carried tail lies in front
TILE = 4096         # ING_TILE: bytes per block of the newline kernels, counted from the buffer's start
SCAN_BLOCK = 1024   # ING_SCAN_BLOCK: elements per block of the two-level scans; level 2 is one wavefront of 64 lanes
SUB = 1 << 20       # reads per launch of a ragged chunk (sub_pairs[r >> 20])


def cap_reads(max_text):
    return max_text // 32 + 1024


def cap_lines(max_text):
    return 4 * cap_reads(max_text) + 8


def n_tiles(submitted_bytes):
    """Tiles the newline kernels run over for a text chunk of that many bytes (whatever is carried lies inside the first 256)."""
    return (CARRY + submitted_bytes + TILE - 1) // TILE


def scan_blocks(n):
    return (n + SCAN_BLOCK - 1) // SCAN_BLOCK


def level2_per(n_blk):
    """Blocks each lane of ing_scan_level2 adds up serially."""
    return (n_blk + 63) // 64


def level2_busy_lanes(n_blk):
    """(lanes with `per` blocks, blocks of the one partly filled lane behind them); the lanes after those are empty."""
    per = level2_per(n_blk)
    return n_blk // per, n_blk % per


# ---- the generator ---------------------------------------------------------------------------------------------------------
Generated = namedtuple("Generated", "text seqs starts")  # bytes; the reads as str; where record i starts in text (n + 1 entries)


def lengths(seed, n, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi + 1, n).astype(np.int64)


def generate(kind, lens, seed, wrap=0):
    """kind "fastq": '@', bases, '+', as many 'I' — a record of 2 L + 6 bytes; "fasta": '>' and the bases in lines of `wrap`
    (0: one line); "lines": the bases. Every line ends in '\\n'. lens >= 1."""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.ndim == 1 and lens.size and lens.min() >= 1
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(lens)])
    total = int(offs[-1])
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, total, dtype=np.uint8)]
    within = np.arange(total, dtype=np.int64) - np.repeat(offs[:-1], lens)  # a base's place in its read

    def laid_out(rec_len, fill, first_base, stride):
        starts = np.concatenate([[0], np.cumsum(rec_len)])
        out = np.full(int(starts[-1]), ord(fill), dtype=np.uint8)
        out[np.repeat(starts[:-1] + first_base, lens) + within + (within // stride if stride else 0)] = bases
        return out, starts

    plain, _ = laid_out(lens + 1, "\n", 0, 0)  # one read per line: the LINES file, and the reads themselves
    seqs = plain[:-1].tobytes().decode("ascii").split("\n")
    if kind == "lines":
        out, starts = plain, np.concatenate([[0], np.cumsum(lens + 1)])
    elif kind == "fasta":
        w = wrap if wrap else int(lens.max())
        out, starts = laid_out(2 + lens + (lens + w - 1) // w, "\n", 2, w)
        out[starts[:-1]] = ord(">")
    else:
        assert kind == "fastq"
        out, starts = laid_out(2 * lens + 6, "I", 2, 0)
        s = starts[:-1]
        out[s] = ord("@")
        out[s + 3 + lens] = ord("+")
        for at in (s + 1, s + 2 + lens, s + 4 + lens, s + 5 + 2 * lens):
            out[at] = ord("\n")
    return Generated(out.tobytes(), seqs, starts)


# ---- the reference parse ---------------------------------------------------------------------------------------------------
def parse_fastq(data: bytes):
    """Split at '\\n', ONE trailing '\\r' dropped, line 2 of every 4."""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    picked = lines[1::4]
    if b"\r" in data:
        picked = [p[:-1] if p.endswith(b"\r") else p for p in picked]
    return b"\n".join(picked).decode("latin-1").split("\n") if picked else []


def parse(kind, data: bytes):
    return parse_fastq(data) if kind == "fastq" else parse_seq(kind, data)


def expected_sub_pairs(offsets, n_reads, uniform_len=0):
    """gmx_ingest_result.sub_pairs from the reads' base offsets: the plane word at which read i << 20 starts."""
    if uniform_len:
        return [(i << 20) * ((uniform_len + 31) // 32) for i in range(16)]
    out = [0] * 16
    for i in range(16):
        if i << 20 < n_reads:
            out[i] = (int(offsets[i << 20]) >> 5) + (i << 20)
    return out


# ---- the sizes of the GPU tests (the host test checks that each reaches its branch) --------------------------------------------
TILE_MAX_TEXT = 8 << 20
TILE_READS_TWO = 29500    # FASTQ, reads of 100-150: about 7.1 MiB behind a first chunk of 64 KiB + 17 bytes, more than 2048 tiles
TILE_FIRST_CUT = (1 << 16) + 17

LEVEL2_MAX_TEXT = 8 << 20
LEVEL2_READS = (70000, 65 * 1024 + 1, 129 * 1024 + 5)  # 69 scan blocks (per 2, a lane half filled), 66 (per 2, none), 130 (per 3)
LEVEL2_CUT_BEFORE_END = 37   # the two-chunk form cuts inside the 37th record from the end

MILLION_MAX_TEXT = 32 << 20
MILLION_READS = SUB + 700
MILLION_SEED = 5
UNIFORM_LEN = 33
UNIFORM_MAX_TEXT = 35 << 20  # 2^20 + 700 lines of 33 bases and '\n' are 35.7 MB: no format puts them into 32 MiB


def tile_file():
    """FASTQ, reads of 100-150, cut behind the first record that ends past 3 MiB: 1025 tiles."""
    g = generate("fastq", lengths(1, 12600, 100, 150), 2)
    k = int(np.searchsorted(g.starts, (3 << 20) + 1))
    return Generated(g.text[:int(g.starts[k])], g.seqs[:k], g.starts[:k + 1])


def tile_file_two_chunks():
    return generate("fastq", lengths(3, TILE_READS_TWO, 100, 150), 4)


def level2_file(kind, n):
    return generate(kind, lengths(n, n, 1, 40), n + 1, wrap=7 if kind == "fasta" else 0)


def level2_cut(g):
    """A byte inside the record LEVEL2_CUT_BEFORE_END from the end (never its first)."""
    return int(g.starts[-1 - LEVEL2_CUT_BEFORE_END]) + 3


def million_file(kind):
    return generate(kind, lengths(MILLION_SEED, MILLION_READS, 5, 12), MILLION_SEED + 1)


def uniform_file():
    return generate("lines", np.full(MILLION_READS, UNIFORM_LEN), 9)


# ---- capacities ------------------------------------------------------------------------------------------------------------
CAP_MAX_TEXT = 1 << 16
Case = namedtuple("Case", "name kind text final fits seqs carried site")
# fits: status 0 and `seqs` are the chunk's reads (carried: bytes of the record left for the next chunk); else status 8 alone.
# site: the test that decides — "tile" gmx_tile_scan2_kernel, "records" ing_records, "lines2" gmx_seq_lines2_kernel.


def capacity_cases():
    cr, cl = cap_reads(CAP_MAX_TEXT), cap_lines(CAP_MAX_TEXT)
    out = []
    for n in (cr, cr + 1):
        g = generate("fastq", lengths(n, n, 1, 4), 11)
        out.append(Case(f"fastq-{n}-reads", "fastq", g.text, True, n <= cr, g.seqs, 0, "records"))
        g = generate("lines", lengths(n, n, 1, 8), 12)
        out.append(Case(f"lines-{n}-reads", "lines", g.text, True, n <= cr, g.seqs, 0, "lines2"))
    # LINES: cap_reads reads among empty lines, which the format ignores — three behind every read, the rest in front
    g = generate("lines", lengths(13, cr, 1, 8), 13)
    for newlines in (cl, cl + 1):
        text = b"\n" * (newlines - 4 * cr) + b"".join(s.encode() + b"\n\n\n\n" for s in g.seqs)
        out.append(Case(f"lines-{newlines}-newlines", "lines", text, True, newlines <= cl, g.seqs, 0, "tile"))
    # ... and a last read without its newline behind cap_lines of them: cap_lines + 1 lines, the last entries of the lines' tables
    text = b"\n" * (cl - 4 * cr + 4) + b"".join(s.encode() + b"\n\n\n\n" for s in g.seqs[:-1]) + g.seqs[-1].encode()
    out.append(Case(f"lines-{cl}-newlines-and-an-open-line", "lines", text, True, True, g.seqs, 0, "lines2"))
    for final, heads in ((False, cr + 1), (False, cr + 2), (True, cr), (True, cr + 1)):
        g = generate("fasta", lengths(heads, heads, 1, 6), 14, wrap=3)
        n = heads if final else heads - 1  # the last head's record goes on in the next chunk
        out.append(Case(f"fasta-{heads}-heads-{'final' if final else 'not-final'}", "fasta", g.text, final, n <= cr, g.seqs[:n],
                        0 if final else int(g.starts[-1] - g.starts[-2]), "lines2"))
    return out


def small_good_file(kind):
    return generate(kind, lengths(21, 50, 1, 70), 22, wrap=11 if kind == "fasta" else 0)


# ---- the edge sweep --------------------------------------------------------------------------------------------------------
EDGE_MAX_TEXT = 1 << 16
EDGE_TAILS = tuple(range(18)) + (4095, 4096, 4097)
Edge = namedtuple("Edge", "first second seqs_first seqs_second nl_at end_residue")


def edge_end_residue(t):
    """The second chunk's length modulo 16 for tail t: every residue over t = 0..15."""
    return (5 * t + 3) % 16


def edge_chunks(kind, t, cr):
    """Two chunks of one file. The first ends t bytes into a record longer than a tile, so the second chunk's text starts at
    CARRY - t: every residue modulo 16, and across a tile's edge. The second chunk's own bytes lie at CARRY + j whatever t is:
    its line lengths put a '\\n' at j = 4095 and j = 0 modulo 4096 (nl_at), and its last line has no '\\n' (cr: a '\\r' instead)
    and ends the text at edge_end_residue(t) modulo 16."""
    assert kind in ("fastq", "lines")
    rng = np.random.default_rng(1000 + t)
    seq = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    rec = (lambda s, h="": f"@{h}\n{s}\n+\n{'I' * len(s)}\n") if kind == "fastq" else (lambda s, h="": s + "\n")  # noqa: E731
    seqs_first = [seq(int(n)) for n in rng.integers(1, 60, 40)]
    head = "".join(rec(s) for s in seqs_first)
    long_read = seq(2100 if kind == "fastq" else 4200)
    long_rec = rec(long_read)
    assert len(long_rec) > t
    seqs_second, body = [long_read], long_rec[t:]
    pos = lambda: len(body)  # noqa: E731  (the second chunk's bytes so far)

    def add(s, h=""):
        nonlocal body
        seqs_second.append(s)
        body += rec(s, h)

    def pad_until(target, room):
        while target - pos() > room:
            add(seq(10))
    nl_a = (pos() // TILE + 1) * TILE + TILE - 1  # 4095 modulo 4096
    if kind == "fastq":
        nl_b = nl_a + 1 + TILE                    # 0 modulo 4096
        pad_until(nl_a, 42)
        add(seq(nl_a - pos() - 2))                # the sequence line's newline
        pad_until(nl_b, 44)
        add(seq(nl_b - pos() - 4))                # the '+' line's newline
    else:
        nl_b = nl_a + 1
        pad_until(nl_a, 40)
        add(seq(nl_a - pos()))
        body += "\n"                              # an empty line: newlines at 4095 and 4096
    for _ in range(5):
        add(seq(int(rng.integers(1, 60))))
    r, c = edge_end_residue(t), 1 if cr else 0
    if kind == "fastq":  # the last record is 5 + h + 2 L + c bytes: h, one more header byte, sets the parity
        h = (r - pos() - 5 - c) % 2
        n = ((r - pos() - 5 - c - h) % 16) // 2 + 8
        add(seq(n), "x" * h)
    else:
        add(seq((r - pos() - c) % 16 + 16))
    body = body[:-1] + ("\r" if cr else "")
    return Edge((head + long_rec[:t]).encode(), body.encode(), seqs_first, seqs_second, (nl_a, nl_b), r)

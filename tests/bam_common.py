"""Shared by test_bam_host.py (no GPU) and test_bam_device.py (GPU): a BAM writer, a restatement in Python of the rules by which
a BAM file's records become reads (include/gmx.h, GMX_INGEST_FORMAT_BAM), and the generated files both tests read.

Everything here works on the file's TEXT — the bytes behind the BGZF layer; test_ingest.bgzf wraps them into a file."""
import struct

import numpy as np

from ingest_formats_common import parse_check_line  # noqa: F401  (re-exported: the tests compare `gram _parse_check` lines)

CODES = "=ACMGRSVTWYHKDBN"
CODE_OF = {c: i for i, c in enumerate(CODES)}
COMPLEMENT = [0, 8, 4, 12, 2, 10, 9, 14, 1, 6, 5, 13, 3, 11, 7, 15]  # of a 4-bit code (the reference's table; A<->T, C<->G)
BASE_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


class BamFormatError(Exception):
    """A malformed record; `index` is the record's place in the file."""

    def __init__(self, index, what):
        super().__init__(f"record {index}: {what}")
        self.index = index


def reverse_complement(seq: str) -> str:
    return "".join(BASE_COMPLEMENT[c] for c in reversed(seq))


def record(seq="", flag=0, name="r", qual=None, cigar=(), tags=b"", ref_id=-1, pos=-1, mapq=0, next_ref_id=-1, next_pos=-1, tlen=0):
    """One record as a dict for bam_bytes. `seq` is what the file STORES (a reverse-strand record stores the reverse complement
    of the read as sequenced); `qual`: bytes of len(seq) Phred values, or None for an absent quality string (0xFF)."""
    return dict(seq=seq, flag=flag, name=name, qual=qual, cigar=tuple(cigar), tags=bytes(tags), ref_id=ref_id, pos=pos, mapq=mapq,
                next_ref_id=next_ref_id, next_pos=next_pos, tlen=tlen)


def record_bytes(r) -> bytes:
    seq = r["seq"]
    name = r["name"].encode() + b"\0"
    assert 1 <= len(name) <= 255
    codes = [CODE_OF[c] for c in seq] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
    qual = bytes([0xFF]) * len(seq) if r["qual"] is None else bytes(r["qual"])
    assert len(qual) == len(seq)
    cigar = b"".join(struct.pack("<I", c) for c in r["cigar"])
    body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(seq), r["next_ref_id"],
                       r["next_pos"], r["tlen"]) + name + cigar + packed + qual + r["tags"]
    return struct.pack("<i", len(body)) + body


def header_bytes(refs=(), header_text="") -> bytes:
    text = header_text.encode()
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode() + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out


def bam_bytes(records, refs=(), header_text="") -> bytes:
    """The text of a BAM file: header, then the records."""
    return header_bytes(refs, header_text) + b"".join(record_bytes(r) for r in records)


def header_length(text: bytes) -> int:
    """Bytes the header takes at the start of the text (what the caller of gmx_ingest_set_bam_header finds by inflating the head)."""
    assert text[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", text, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", text, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", text, at)
        at += 4 + l_name + 4
    return at


def parse_bam(text: bytes, with_quals=False):
    """The rules: EVERY record is a read, in file order; the read is the l_seq bases, reversed and complemented when flag & 0x10;
    qualities are 33 + q, reversed with the read. Raises BamFormatError for a malformed record: block_size smaller than its
    fields need, l_read_name == 0, l_seq < 0, or the text ends inside the record."""
    at = header_length(text)
    reads, quals = [], []
    while at < len(text):
        index = len(reads)
        if at + 4 > len(text):
            raise BamFormatError(index, "the text ends inside block_size")
        block_size, = struct.unpack_from("<i", text, at)
        if block_size < 32:
            raise BamFormatError(index, f"block_size {block_size}")
        if at + 36 > len(text):
            raise BamFormatError(index, "the text ends inside the record")
        _, _, l_name, _, _, n_cigar, flag, l_seq, _, _, _ = struct.unpack_from("<iiBBHHHiiii", text, at + 4)
        if l_name == 0 or l_seq < 0 or block_size < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:
            raise BamFormatError(index, f"block_size {block_size}, l_read_name {l_name}, n_cigar_op {n_cigar}, l_seq {l_seq}")
        if at + 4 + block_size > len(text):
            raise BamFormatError(index, "the text ends inside the record")
        seq_at = at + 36 + l_name + 4 * n_cigar
        codes = [(text[seq_at + i // 2] >> 4) if i % 2 == 0 else (text[seq_at + i // 2] & 15) for i in range(l_seq)]
        qual = list(text[seq_at + (l_seq + 1) // 2:seq_at + (l_seq + 1) // 2 + l_seq])
        if flag & 0x10:
            codes = [COMPLEMENT[c] for c in reversed(codes)]
            qual.reverse()
        reads.append("".join(CODES[c] for c in codes))
        quals.append(bytes((33 + q) & 0xFF for q in qual))
        at += 4 + block_size
    return (reads, quals) if with_quals else reads


def _seq(rng, n, letters="ACGT"):
    return "".join(letters[c] for c in rng.integers(0, len(letters), n))


def _quals(rng, n):
    return bytes(int(q) for q in rng.choice([2, 12, 23, 37], n))


def fake_record_bytes(rng, l_seq=20) -> bytes:
    """A complete, plausible record — to be hidden inside another record's tag."""
    return record_bytes(record(_seq(rng, l_seq), name="fake", qual=_quals(rng, l_seq), ref_id=0, pos=5))


def b_tag(tag: bytes, payload: bytes) -> bytes:
    """An array tag of bytes (`B`, subtype `C`)."""
    return tag + b"BC" + struct.pack("<i", len(payload)) + payload


def z_tag(tag: bytes, payload: bytes) -> bytes:
    return tag + b"Z" + payload + b"\0"


def trap_records(rng, n=400):
    """Records whose LAST tag holds complete plausible records right in front of the next record's start. A tile that starts inside
    such a tag speculates from a fake record; the fake chain either runs into a bare block_size that leads nowhere (odd records)
    or ends exactly on the next real record (even records: the tile's exit is right and its records are not)."""
    out = []
    for i in range(n):
        seq = _seq(rng, int(rng.integers(1, 90)))
        fakes = b"".join(fake_record_bytes(rng, int(rng.integers(0, 30))) for _ in range(int(rng.integers(2, 6))))
        stray = struct.pack("<i", int(rng.integers(33, 200))) + struct.pack("<i", -1)  # a block_size and a refID with nothing behind them
        tags = z_tag(b"XZ", b"some text")
        if i % 3 == 0:
            tags += b_tag(b"XA", bytes(int(rng.integers(0, 64))) + fakes[:int(rng.integers(40, 90))])
        tags += b_tag(b"XB", fakes + (stray if i % 2 else b""))
        out.append(record(seq, flag=0x10 if i % 2 else 0, name=f"trap{i}", qual=_quals(rng, len(seq)), tags=tags))
    return out


def generated_files():
    """(name, text): the files both tests read. Every one is well-formed."""
    rng = np.random.default_rng(4321)
    refs2 = [("chr1", 100000), ("chr2", 5000)]
    out = []

    def add(name, records, refs=refs2, header_text="@HD\tVN:1.6\tSO:unsorted\n"):
        out.append((name, bam_bytes(records, refs, header_text)))

    add("uniform-100", [record(_seq(rng, 100), flag=0x10 if i % 2 else 0, name=f"u{i}", qual=_quals(rng, 100)) for i in range(300)])
    add("ragged-1-259", [record(_seq(rng, int(k)), flag=0x10 if i % 3 == 0 else 0, name=f"read{i}/1", qual=_quals(rng, int(k)), cigar=(int(k) << 4,),
                                ref_id=i % 2, pos=i * 7) for i, k in enumerate(rng.integers(1, 260, 300))])
    add("tiny-1-3", [record(_seq(rng, int(k)), flag=0x10 if i % 2 else 0, name=f"t{i}", qual=_quals(rng, int(k))) for i, k in enumerate(rng.integers(1, 4, 400))])
    add("empty-reads", [record("" if i % 3 else _seq(rng, 33), flag=0x10 if i % 4 == 1 else 0, name=f"e{i}", qual=None if i % 3 else _quals(rng, 33)) for i in range(200)])
    add("all-empty", [record("", name=f"z{i}") for i in range(5)])
    flags = [a | b | c | d for a in (0, 0x10) for b in (0, 0x100) for c in (0, 0x800) for d in (0, 0x4)]
    add("flag-mixes", [record(_seq(rng, 20 + i % 50), flag=flags[i % 16], name=f"f{i}", qual=_quals(rng, 20 + i % 50)) for i in range(320)])
    add("odd-even-both-strands", [record(_seq(rng, n), flag=fl, name=f"p{n}", qual=_quals(rng, n)) for n in list(range(1, 70)) + [95, 96, 97, 127, 128, 129, 160, 161]
                                  for fl in (0, 0x10)])
    odd = []
    for i in range(300):
        n = int(rng.integers(1, 200))
        s = _seq(rng, n)
        if i % 4 == 1:
            k = int(rng.integers(0, n))
            s = s[:k] + "N" + s[k + 1:]
        elif i % 4 == 2:
            k = int(rng.integers(0, n))
            s = s[:k] + "=" + s[k + 1:]
        elif i % 4 == 3:
            s = _seq(rng, n, CODES if i % 8 == 3 else "ACGTMRSVWYHKDB")
        odd.append(record(s, flag=0x10 if i % 3 == 1 else 0, name=f"o{i}", qual=_quals(rng, n)))
    add("n-equals-iupac", odd)
    add("absent-qualities", [record(_seq(rng, int(k)), flag=0x10 if i % 2 else 0, name=f"q{i}", qual=None) for i, k in enumerate(rng.integers(1, 150, 200))])
    add("long-names-many-cigar-ops", [record(_seq(rng, int(k)), flag=0x10 if i % 2 else 0, name="n" * (254 if i % 2 else 1 + i % 250), qual=_quals(rng, int(k)),
                                             cigar=[(1 + j % 9) << 4 | j % 9 for j in range(i % 7 * 40)]) for i, k in enumerate(rng.integers(1, 120, 120))])
    add("large-tags", [record(_seq(rng, int(k)), flag=0x10 if i % 2 else 0, name=f"g{i}", qual=_quals(rng, int(k)),
                              tags=b_tag(b"XL", bytes(rng.integers(0, 256, int(rng.integers(0, 9000)), dtype=np.uint8))) + z_tag(b"RG", b"group"))
                       for i, k in enumerate(rng.integers(1, 160, 30))])
    add("one-read-of-300k", [record(_seq(rng, 70), name="a", qual=_quals(rng, 70)), record(_seq(rng, 300001), flag=0x10, name="long", qual=_quals(rng, 300001)),
                             record(_seq(rng, 31), flag=0x10, name="b", qual=_quals(rng, 31))])
    add("header-of-700-references", [record(_seq(rng, int(k)), flag=0x10 if i % 2 else 0, name=f"h{i}", qual=_quals(rng, int(k)), ref_id=i % 700)
                                     for i, k in enumerate(rng.integers(1, 259, 200))],
        refs=[(f"contig_{i}_of_an_assembly", 1000 + i) for i in range(700)], header_text="@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:contig_{i}_of_an_assembly\tLN:{1000 + i}\n" for i in range(700)))
    add("header-only", [])
    add("no-references", [record(_seq(rng, 50), name=f"x{i}", qual=_quals(rng, 50)) for i in range(20)], refs=(), header_text="")
    add("tag-traps", trap_records(rng, 150))
    return out


def malformed_texts():
    """(kind, text, index of the malformed record): one file for each of the four kinds."""
    rng = np.random.default_rng(99)
    good = [record(_seq(rng, 40), name=f"m{i}", qual=_quals(rng, 40), flag=0x10 if i % 2 else 0) for i in range(30)]
    head = bam_bytes(good[:17], [("chr1", 1000)])
    rest = b"".join(record_bytes(r) for r in good[18:])
    victim = bytearray(record_bytes(good[17]))
    out = []
    short = bytearray(victim)
    struct.pack_into("<i", short, 0, 32 + 4 + 10)  # block_size too small for name + seq + qual
    out.append(("block-size-too-small", head + bytes(short) + rest, 17))
    noname = bytearray(victim)
    noname[12] = 0
    out.append(("no-read-name", head + bytes(noname) + rest, 17))
    neg = bytearray(victim)
    struct.pack_into("<i", neg, 20, -5)
    out.append(("negative-l-seq", head + bytes(neg) + rest, 17))
    whole = head + bytes(victim)
    out.append(("text-ends-inside-a-record", whole[:-9], 17))
    return out


def stats_reads(seed=8, n=60):
    """Reads with qualities for the base-error-rate check: (sequenced read, Phred bytes in sequencing order)."""
    rng = np.random.default_rng(seed)
    return [(_seq(rng, int(k)), bytes(int(q) for q in rng.integers(2, 41, int(k)))) for k in rng.integers(5, 80, n)]

"""Shared by test_ingest_formats.py (GPU) and test_ingest_formats_host.py (no GPU): generated FASTA / one-read-per-line files and
a restatement in Python of the two formats' rules (include/gmx.h, gmx_ingest_set_format), which are those of `gram`'s general
host reader (SeqReader::next)."""
import numpy as np


def lines_of(data: bytes):
    """The file's lines as the reader sees them: ended by '\\n' (a last line may lack it), ONE '\\r' in front of it dropped."""
    parts = data.split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def parse_fasta(data: bytes):
    """A read per '>' line: every line up to the next '>' line put together (blank lines add nothing; an empty read counts)."""
    reads = []
    for line in lines_of(data):
        if line[:1] == b">":
            reads.append(b"")
        elif line:
            assert reads, "sequence in front of the first header: not a FASTA file"
            reads[-1] += line
    return [r.decode("latin-1") for r in reads]


def parse_lines(data: bytes):
    """Every non-empty line is a read."""
    return [line.decode("latin-1") for line in lines_of(data) if line]


def parse(kind: str, data: bytes):
    return parse_fasta(data) if kind == "fasta" else parse_lines(data)


def parse_check_line(seqs):
    """"<n_reads> <n_bases> <FNV-1a>" as `gram _parse_check` prints it: 64-bit offsets (the leading 0 included), then the bases
    1..4 as 64-bit values; an unencodable read is the empty read."""
    mask = (1 << 64) - 1
    prime = 1099511628211
    prime7 = pow(prime, 7, 1 << 64)  # (seven zero bytes behind a base's own)
    code = {c: v for c, v in zip("ACGTacgt", (1, 2, 3, 4, 1, 2, 3, 4))}
    kept = [s if all(c in code for c in s) else "" for s in seqs]
    h = 1469598103934665603
    at = 0
    for s in [None] + kept:
        at += len(s) if s is not None else 0
        for i in range(8):
            h = ((h ^ ((at >> (8 * i)) & 0xFF)) * prime) & mask
    for s in kept:
        for c in s:
            h = ((((h ^ code[c]) * prime) & mask) * prime7) & mask
    return f"{len(seqs)} {at} {h}"


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _wrap(s, width, nl):
    return "".join(s[i:i + width] + nl for i in range(0, len(s), width)) if width else s + nl


def fasta_text(seqs, width=0, nl="\n", final_newline=True):
    text = "".join(f">read{i} d:{i * 7919}{nl}{_wrap(s, width, nl) if s else ''}" for i, s in enumerate(seqs))
    return (text if final_newline else text[:len(text) - len(nl)]).encode()


def generated_files(n=300):
    """(name, kind, bytes): the files of the C-ABI test. Every one must be accepted by the device."""
    rng = np.random.default_rng(77)
    ragged = [_seq(rng, int(k)) for k in rng.integers(1, 260, n)]
    short = [_seq(rng, int(k)) for k in rng.integers(1, 41, n)]
    uniform = [_seq(rng, 100) for _ in range(n)]
    out = [("fa-single-uniform", "fasta", fasta_text(uniform)),
           ("fa-single-ragged", "fasta", fasta_text(ragged)),
           ("fa-wrap60-uniform", "fasta", fasta_text(uniform, 60)),
           ("fa-wrap60", "fasta", fasta_text(ragged, 60)),
           ("fa-wrap1", "fasta", fasta_text(short, 1)),
           ("fa-wrap31", "fasta", fasta_text(ragged, 31)),
           ("fa-wrap32", "fasta", fasta_text(ragged, 32)),
           ("fa-wrap33", "fasta", fasta_text(ragged, 33)),
           ("fa-crlf", "fasta", fasta_text(ragged, 70, nl="\r\n")),
           ("fa-no-final-newline", "fasta", fasta_text(ragged, 60, final_newline=False)),
           ("fa-crlf-no-final-newline", "fasta", fasta_text(ragged, 0, nl="\r\n")[:-1])]  # (ends in '\r': stripped at the file's end too)
    odd = []  # lower case, N, a blank inside a sequence, a sequence line that starts with '@' or '+'
    for i, s in enumerate(ragged):
        if i % 3 == 0:
            s = s.lower()
        if i % 7 == 3:
            k = int(rng.integers(0, len(s)))
            s = s[:k] + "N" + s[k + 1:]
        if i % 11 == 5 and len(s) > 2:
            k = int(rng.integers(1, len(s) - 1))
            s = s[:k] + " " + s[k + 1:]
        if i % 13 == 6:
            s = "@+"[i % 2] + s
        odd.append(s)
    out.append(("fa-odd-letters", "fasta", fasta_text(odd, 45)))
    blanks = ["\n\r\n\n"]  # leading blank lines; blank lines between and inside records; empty records in the middle and at the end
    for i, s in enumerate(ragged):
        if i % 17 == 4:
            s = ""
        body = _wrap(s, 50, "\n") if s else ""
        if i % 5 == 1 and len(s) > 50:
            body = body.replace("\n", "\n\n", 1)
        if i % 6 == 2:
            body = "\n" + body
        blanks.append(f">r{i}\n{body}" + ("\n\r\n" if i % 4 == 0 else ""))
    blanks.append(">last-and-empty\n")
    out.append(("fa-blank-lines-empty-records", "fasta", "".join(blanks).encode()))
    out.append(("fa-all-empty", "fasta", b">a\n>b\n\n>c\n"))
    out.append(("ln-uniform", "lines", "".join(s + "\n" for s in uniform).encode()))
    out.append(("ln-ragged-blank-lines", "lines", ("\n" + "".join(s + ("\n\n" if i % 5 == 0 else "\n") for i, s in enumerate(ragged))).encode()))
    out.append(("ln-crlf", "lines", "".join(s + ("\r\n\r\n" if i % 9 == 0 else "\r\n") for i, s in enumerate(ragged)).encode()))
    out.append(("ln-odd-letters-no-final-newline", "lines", "\n".join(s.lstrip("@+") or "A" for s in odd).encode()))
    return out


def cli_reads(n, seed):
    """Reads as tests/test_ingest.py's _cli_fastq makes them: 1-259 bases, every ninth with Ns."""
    rng = np.random.default_rng(seed)
    return ["".join("ACGTN"[int(x)] for x in rng.integers(0, 5 if i % 9 == 0 else 4, size=int(rng.integers(1, 260)))) for i in range(n)]


def gram(*args, env=None):
    import os
    import subprocess
    from gramtools_amd.build import build_gram
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([build_gram(), *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=e)


def parse_check_lines(out):
    return {l.split()[0]: " ".join(l.split()[1:]) for l in out.stdout.strip().splitlines() if l.split() and l.split()[0] in ("fast", "slow", "device")}

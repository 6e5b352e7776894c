"""FASTA and one-read-per-line reads files on the device (gmx_ingest_set_format): `gram genotype` on one set of
reads written several ways, device route against the host's general reader.
Usage:
  python tools/fasta_device_bench.py make DIR [n_reads [FORMATS]]   n x 150-base reads as fa1 (single-line FASTA), fa60 (wrapped at 60), lines
                                                          (one read per line) and fq (four-line FASTQ), each as plain text, BGZF at
                                                          level 6 (.bgz) and ONE gzip stream at level 6 (.gz), and a PRG -> DIR
  python tools/fasta_device_bench.py gram DIR NAME THREADS [reps]   `gram genotype --max_threads THREADS` on DIR/NAME: the device route
                                                          and the host reader (GMX_HOST_FASTQ=1 GMX_HOST_GZ=1) alternated; wall
                                                          seconds and the quasimap phase
Each call is one process: a job script runs them one after the other, each under its own time limit."""
import os
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMATS = ("fa1", "fa60", "lines", "fq")


def _text(fmt, seed, first, n):
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 150))]
    out = []
    for i in range(n):
        s = bases[i].tobytes().decode()
        if fmt == "fa1":
            out.append(f">read{first + i}\n{s}\n")
        elif fmt == "fa60":
            out.append(f">read{first + i}\n{s[:60]}\n{s[60:120]}\n{s[120:]}\n")
        elif fmt == "lines":
            out.append(s + "\n")
        else:
            out.append(f"@read{first + i}\n{s}\n+\n{'I' * 150}\n")
    return "".join(out).encode()


def _slice(args):
    fmt, seed, first, n, last = args
    text = _text(fmt, seed, first, n)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    gz = c.compress(text) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)
    bg = bytearray()
    for at in range(0, len(text), 65280):
        piece = text[at:at + 65280]
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
        comp = c.compress(piece) + c.flush()
        bg += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1)
        bg += comp + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece))
    return text, gz, bytes(bg)


def make(d, n, formats=FORMATS):
    os.makedirs(d, exist_ok=True)
    step = 125000
    with ProcessPoolExecutor(16) as ex:
        for fmt in formats:
            jobs = [(fmt, 1000 + i, i, min(step, n - i), i + step >= n) for i in range(0, n, step)]  # (the same reads in every format)
            crc, size = 0, 0
            p = os.path.join(d, "r." + fmt)
            with open(p, "wb") as ft, open(p + ".gz", "wb") as fg, open(p + ".bgz", "wb") as fb:
                fg.write(b"\x1f\x8b\x08\x00\0\0\0\0\0\x03")
                for text, gz, bg in ex.map(_slice, jobs):
                    crc = zlib.crc32(text, crc)
                    size += len(text)
                    ft.write(text)
                    fg.write(gz)
                    fb.write(bg)
                fg.write((crc & 0xFFFFFFFF).to_bytes(4, "little") + (size & 0xFFFFFFFF).to_bytes(4, "little"))
                fb.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
            print(f"{fmt}: {n} reads, {size / 1e6:.0f} MB of text, {os.path.getsize(p + '.gz') / 1e6:.0f} MB gzip, {os.path.getsize(p + '.bgz') / 1e6:.0f} MB BGZF", flush=True)
    from gramtools_amd.synth import random_ref, snp_prg
    ref = random_ref(1000000, 7)
    prg, *_ = snp_prg(ref, 15000, 2)
    np.array(prg, dtype="<u4").tofile(os.path.join(d, "prg"))


def gram(d, name, threads, reps):
    from gramtools_amd.build import build_gram
    g = build_gram()
    for rep in range(reps):
        for route, env in (("device", {}), ("host", {"GMX_HOST_FASTQ": "1", "GMX_HOST_GZ": "1"})):
            out = os.path.join(d, f"out_{name}_{route}")
            t0 = time.perf_counter()
            r = subprocess.run([g, "genotype", "--gram_dir", d, "--reads", os.path.join(d, name), "--sample_id", "s", "--ploidy", "haploid",
                                "--kmer_size", "10", "--genotype_dir", out, "--seed", "42", "--max_threads", str(threads)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, **env))
            dt = time.perf_counter() - t0
            feed = [l.strip() for l in r.stdout.splitlines() if "Quasimap (" in l or "warning" in l]
            print(f"{name} threads {threads} rep {rep} {route}: rc {r.returncode}, {dt:.2f} s wall; " + " | ".join(feed[-2:]), flush=True)
            if r.returncode:
                print(r.stdout[-2000:])
                sys.exit(1)


if __name__ == "__main__":
    if sys.argv[1] == "make":
        make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4000000, tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else FORMATS)
    else:
        gram(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else 3)

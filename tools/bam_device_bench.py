"""BAM reads files on the device (GMX_INGEST_FORMAT_BAM): the device chain alone, and `gram genotype` on one set
of reads written as BAM and as BGZF FASTQ, device route against the host reader.
Usage:
  python tools/bam_device_bench.py make DIR [n_reads [length]]   n x 150-base (or `length`-base) reads as r.bam (Illumina-style names, binned qualities,
                                                                 every second record reverse-strand, BGZF level 6; written with the
                                                                 tests' writer, tests/bam_common.py) and r.fq.bgz, and a PRG -> DIR
  python tools/bam_device_bench.py chain DIR NAME [reps]         the ingest alone on DIR/NAME (r.bam or r.fq.bgz): upload, inflate, record
                                                                 chain / scan, pack; chunks of 7 168 members over three slots
  python tools/bam_device_bench.py gram DIR NAME THREADS [reps]  `gram genotype --max_threads THREADS` on DIR/NAME: the device route and
                                                                 the host reader (GMX_HOST_GZ=1) alternated; wall seconds, quasimap phase
Each call is one process: a job script runs them one after the other, each under its own time limit."""
import os
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _members(text):
    bg = bytearray()
    for at in range(0, len(text), 65280):
        piece = text[at:at + 65280]
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
        comp = c.compress(piece) + c.flush()
        bg += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1)
        bg += comp + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece))
    return bytes(bg)


def _slice(args):
    from bam_common import header_bytes, record, record_bytes, reverse_complement
    seed, first, n, length = args
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, length))]
    quals = np.array([2, 12, 23, 37], dtype=np.uint8)[rng.integers(0, 4, (n, length))]
    bam = [header_bytes([("chr1", 1000000)], "@HD\tVN:1.6\tSO:unsorted\n")] if first == 0 else []
    fq = []
    for i in range(n):
        s, q = bases[i].tobytes().decode(), quals[i].tobytes()
        name = f"A00123:45:HXXXXDSXX:{1 + (first + i) % 4}:{1101 + (first + i) // 100000}:{(first + i) % 31000}:{(first + i) % 47000}"
        back = (first + i) % 2 == 1
        bam.append(record_bytes(record(reverse_complement(s) if back else s, flag=0x10 if back else 0, name=name, qual=q[::-1] if back else q,
                                       cigar=(length << 4,), ref_id=0, pos=(first + i) % 900000, mapq=60)))
        fq.append(f"@{name}\n{s}\n+\n{bytes(33 + v for v in q).decode()}\n")
    bam, fq = b"".join(bam), "".join(fq).encode()
    return len(bam), _members(bam), len(fq), _members(fq)


def make(d, n, length):
    os.makedirs(d, exist_ok=True)
    step = max(1, 62500 * 150 // length)
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    with ProcessPoolExecutor(16) as ex, open(os.path.join(d, "r.bam"), "wb") as fb, open(os.path.join(d, "r.fq.bgz"), "wb") as fq:
        tb = tq = 0
        for nb, b, nq, q in ex.map(_slice, [(1000 + i, i, min(step, n - i), length) for i in range(0, n, step)]):
            tb += nb
            tq += nq
            fb.write(b)
            fq.write(q)
        fb.write(eof)
        fq.write(eof)
    print(f"{n} reads of {length} bases: r.bam {tb / 1e6:.0f} MB of text, {os.path.getsize(os.path.join(d, 'r.bam')) / 1e6:.0f} MB BGZF; "
          f"r.fq.bgz {tq / 1e6:.0f} MB of text, {os.path.getsize(os.path.join(d, 'r.fq.bgz')) / 1e6:.0f} MB BGZF", flush=True)
    from gramtools_amd.synth import random_ref, snp_prg
    ref = random_ref(1000000, 7)
    prg, *_ = snp_prg(ref, 15000, 2)
    np.array(prg, dtype="<u4").tofile(os.path.join(d, "prg"))


def chain(d, name, reps):
    from gramtools_amd import Ingest, bgzf_members, PinnedArray
    raw = open(os.path.join(d, name), "rb").read()
    mem = [m for m in bgzf_members(raw) if m[2]]
    per = 7168
    chunks = []
    for i in range(0, len(mem), per):
        ch = mem[i:i + per]
        lo, hi = ch[0][0], ch[-1][0] + ch[-1][1]
        pin = PinnedArray(hi - lo, np.uint8)
        pin.array[:] = np.frombuffer(raw, dtype=np.uint8, count=hi - lo, offset=lo)
        chunks.append((pin, Ingest.member_array([(o - lo, s, t, c) for o, s, t, c in ch])))
    ing = Ingest(max_text_bytes=per * 65536 + 65536)
    is_bam = name.endswith(".bam")
    header = 0
    if is_bam:
        from gramtools_amd import GMX_INGEST_FORMAT_BAM
        from bam_common import header_length
        header = header_length(zlib.decompress(raw[:mem[0][0] + mem[0][1]][mem[0][0]:], -15))
        ing.set_format(GMX_INGEST_FORMAT_BAM)
    for rep in range(reps + 1):  # (the first pass warms up)
        ing.reset()
        if is_bam:
            ing.set_bam_header(header)
        t0 = time.perf_counter()
        reads, k = 0, 0
        for k in range(min(2, len(chunks))):
            ing.submit_bgzf(k % 3, chunks[k][0].array, chunks[k][1], k == len(chunks) - 1)
        for ci in range(len(chunks)):
            if ci + 2 < len(chunks):
                ing.submit_bgzf((ci + 2) % 3, chunks[ci + 2][0].array, chunks[ci + 2][1], ci + 2 == len(chunks) - 1)
            res = ing.wait(ci % 3)
            assert res.status == 0, res.status
            reads += int(res.n_reads)
        dt = time.perf_counter() - t0
        print(f"chain {name} pass {rep}{' (warm-up)' if rep == 0 else ''}: {reads} reads in {dt * 1e3:.1f} ms = {reads / dt / 1e6:.1f} M reads/s"
              + (f", {ing.bam_rewalks()} tiles walked again so far" if is_bam else ""), flush=True)
    ing.close()


def gram(d, name, threads, reps):
    from gramtools_amd.build import build_gram
    g = build_gram()
    for rep in range(reps):
        for route, env in (("device", {}), ("host", {"GMX_HOST_GZ": "1"})):
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
        make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4000000, int(sys.argv[4]) if len(sys.argv) > 4 else 150)
    elif sys.argv[1] == "chain":
        chain(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    else:
        gram(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]) if len(sys.argv) > 5 else 3)

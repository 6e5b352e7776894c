"""Quality trimming in the device feed (`gram genotype --trim_quality`): what it costs and what it buys on a
BGZF FASTQ with realistic qualities. profiles/quality_trim/README.md holds the numbers and the command lines.
Usage:
  python tools/quality_trim_bench.py make DIR [n_reads]        n x 150-base reads drawn from a SNP PRG of 1 M bases (Illumina-style names,
                                                               binned qualities; about 15 % of the reads with a tail of quality 2 of 5..60
                                                               bases that holds miscalled bases and Ns) as DIR/r.fq.bgz, the PRG and its index
  python tools/quality_trim_bench.py gram DIR GRAM LABEL [gram genotype flags ...]
                                                               one `GRAM genotype` call on DIR/r.fq.bgz (GRAM: a `gram` executable, this tree's
                                                               or another build's): wall seconds, the quasimap phase, reads/s, the counters
  python tools/quality_trim_bench.py kernels CSV               the ingest kernels' rows of a rocprofv3 `--kernel-trace --stats` kernel_stats.csv
Each call is one process: a job script alternates the builds, each call under its own time limit."""
import csv
import os
import re
import struct
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 150


def _slice(args):
    seed, first, reads = args
    rng = np.random.default_rng(seed)
    n = reads.shape[0]
    codes = reads.copy()
    lvl = np.frombuffer(b"F:,", dtype=np.uint8)
    q = lvl[np.repeat(rng.choice(3, size=(n, L // 5), p=[0.92, 0.06, 0.02]), 5, axis=1)]
    poor = np.nonzero(rng.random(n) < 0.15)[0]
    for i in poor:  # a tail the sequencer gave up on: quality 2, a tenth of its bases miscalled, now and then an N
        k = int(rng.integers(5, 61))
        q[i, L - k:] = ord("#")
        wrong = L - k + np.nonzero(rng.random(k) < 0.1)[0]
        codes[i, wrong] = (codes[i, wrong] - 1 + rng.integers(1, 4, wrong.size)) % 4 + 1
        if rng.random() < 0.3:
            codes[i, L - 1 - int(rng.integers(0, k))] = 0
    bases = np.frombuffer(b"NACGT", dtype=np.uint8)[codes]
    xs, ys = rng.integers(1000, 30000, n), rng.integers(1000, 30000, n)
    text = b"".join(b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT\n%s\n+\n%s\n" % (1101 + (first + i) // 40000, xs[i], ys[i], bases[i].tobytes(), q[i].tobytes())
                    for i in range(n))
    out = bytearray()
    for at in range(0, len(text), 65280):
        p = text[at:at + 65280]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(p) + c.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(comp) + 8 - 1)
        out += comp + struct.pack("<II", zlib.crc32(p) & 0xFFFFFFFF, len(p))
    return bytes(out), len(text), len(poor)


def make(d, n):
    from gramtools_amd.build import build_gram
    from gramtools_amd.synth import random_ref, simulate_snp_reads_fast, snp_prg
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    ref = random_ref(1000000, 7)
    prg, pos, alts, n_alts = snp_prg(ref, 15000, 2)
    np.array(prg, dtype="<u4").tofile(os.path.join(d, "prg"))
    reads = simulate_snp_reads_fast(ref, pos, alts, n_alts, n, L, 1000)
    per = 62500
    text = poor = 0
    with ProcessPoolExecutor(16) as ex, open(os.path.join(d, "r.fq.bgz"), "wb") as fh:
        for part, t, p in ex.map(_slice, [(7 + i, i * per, reads[i * per:(i + 1) * per]) for i in range((n + per - 1) // per)]):
            fh.write(part)
            text += t
            poor += p
        fh.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    print(f"{n} reads of {L} bases, {poor} with a poor tail: {text / 1e6:.0f} MB of text, {os.path.getsize(os.path.join(d, 'r.fq.bgz')) / 1e6:.0f} MB of BGZF, "
          f"written in {time.time() - t0:.0f} s", flush=True)
    subprocess.run([build_gram(), "build", "--gram_dir", d, "--kmer_size", "10", "--max_threads", "16"], stdout=subprocess.DEVNULL, check=True)


def gram(d, exe, label, flags):
    out = os.path.join(d, "out_" + label)
    cmd = [exe, "genotype", "--gram_dir", d, "--reads", os.path.join(d, "r.fq.bgz"), "--sample_id", "s", "--ploidy", "haploid", "--kmer_size", "10",
           "--genotype_dir", out, "--max_threads", "16", "--seed", "42"] + list(flags)
    t0 = time.perf_counter()
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=dict(os.environ, GMX_PHASE_TRACE="1"))
    dt = time.perf_counter() - t0
    lines = p.stdout.splitlines()
    if p.returncode:
        print(p.stdout[-2000:])
        sys.exit(1)
    t_map = [float(l.split()[1]) for l in lines if l.startswith("[phase") and ("quasimap done" in l or "base error rate" in l)]
    counts = {l.split(":")[0][6:]: int(l.split(":")[1]) for l in lines if l.startswith("Count ")}
    n = counts["all reads"] // 2  # (the counters include the reverse complements)
    q = (t_map[1] - t_map[0]) / 1e3 if len(t_map) == 2 else float("nan")
    trim = os.path.join(out, "read_trim.json")
    print(f"{label:8s} whole call {dt:.2f} s; reads decoded + mapped in {q * 1e3:.1f} ms = {n / q / 1e6:.1f} M reads/s; orientations exactly mapped {counts['exact mapped reads']}, "
          f"skipped {counts['skipped reads with no sequence']} of {2 * n}" + (("; " + open(trim).read().strip()) if os.path.exists(trim) else ""), flush=True)


def kernels(path):
    for i, r in enumerate(csv.reader(open(path))):
        if i == 0:
            continue
        name = re.sub(r"\(anonymous namespace\)::", "", r[0]).split("(")[0]
        if re.match(r"(void )?gmx_(records|nl_|tile_|layout|offsets|fq_pack|inflate|carry)", name):
            print(f"{name:32s} calls {r[1]:>4s}  avg {float(r[3]) / 1e3:10.1f} us  total {float(r[2]) / 1e6:8.3f} ms  {r[4]:>6s} %")


if __name__ == "__main__":
    if sys.argv[1] == "make":
        make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4000000)
    elif sys.argv[1] == "gram":
        gram(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5:])
    else:
        kernels(sys.argv[2])

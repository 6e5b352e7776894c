"""Plain gzip FASTQ decoded on the device (gmx_ingest_submit_gzip): rate of the device chain and of `gram genotype`.
Usage:
  python tools/gz_device_bench.py make DIR [n_reads]   the 4 M x 150 bp FASTQ of tools/ingest_bench.py as ONE deflate stream at
                                                       level 6 (slices compressed side by side and joined with sync flushes, as pigz
                                                       does) -> DIR/r.fq.gz, and a PRG for `gram` -> DIR/prg
  python tools/gz_device_bench.py chain FILE [reps]    (a) upload, find, decode, link, window, resolve, CRC, record scan, pack: the
                                                       file in chunks of GMX_GZ_CHUNK bytes (32 MB) + 1 MB look-ahead, two chunks on
                                                       the device; reads/s of the whole file, best of reps
  python tools/gz_device_bench.py gram DIR [reps]      (c) `gram genotype --max_threads 1` on DIR/r.fq.gz: the device route and
                                                       GMX_HOST_GZ=1 alternated; wall seconds and the feed's own line
  python tools/gz_device_bench.py host FILE [threads]  (d) the host decoder + parser alone (`gram _parse_bench`)
Each mode is one process: a job script runs them one after the other, each under its own time limit."""
import os
import subprocess
import sys
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _slice(args):
    seed, first, n, last = args
    sys.argv = sys.argv[:1]  # (ingest_bench reads its own arguments when imported)
    import ingest_bench
    text = ingest_bench.make_text(seed, first, n)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    return text, c.compress(text) + c.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)


def make(d, n):
    os.makedirs(d, exist_ok=True)
    step = 250000
    jobs = [(1000 + i, i, min(step, n - i), i + step >= n) for i in range(0, n, step)]
    crc, size = 0, 0
    with open(os.path.join(d, "r.fq.gz"), "wb") as f, ProcessPoolExecutor(16) as ex:
        f.write(b"\x1f\x8b\x08\x00\0\0\0\0\0\x03")
        for text, comp in ex.map(_slice, jobs):
            crc = zlib.crc32(text, crc)
            size += len(text)
            f.write(comp)
        f.write((crc & 0xFFFFFFFF).to_bytes(4, "little") + (size & 0xFFFFFFFF).to_bytes(4, "little"))
    from gramtools_amd.synth import random_ref, snp_prg
    ref = random_ref(1000000, 7)
    prg, *_ = snp_prg(ref, 15000, 2)
    np.array(prg, dtype="<u4").tofile(os.path.join(d, "prg"))
    print(f"made {n} reads: {size / 1e9:.2f} GB of text, {os.path.getsize(os.path.join(d, 'r.fq.gz')) / 1e6:.0f} MB gzip")


def chain(path, reps):
    from gramtools_amd import Ingest
    data = np.fromfile(path, dtype=np.uint8)
    chunk = int(os.environ.get("GMX_GZ_CHUNK", 32 << 20))
    look = 1 << 20
    n = data.size
    ing = Ingest(max_text_bytes=8 * chunk)
    best = None
    for rep in range(reps):
        ing.reset()
        t0 = time.perf_counter()
        reads, waited, k, cuts = 0, 0, 0, list(range(0, n, chunk))
        for k, c0 in enumerate(cuts):
            final = k + 1 == len(cuts)
            own = min(chunk, n - c0)
            ing.submit_gzip(k % 3, data[c0:c0 + own if final else min(n, c0 + own + look)], own, final)
            if k >= 1:
                res = ing.wait((k - 1) % 3)
                assert res.status == 0, f"chunk {k - 1}: status {res.status}"
                reads += res.n_reads
        res = ing.wait(k % 3)
        assert res.status == 0, f"last chunk: status {res.status}"
        reads += res.n_reads
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        print(f"rep {rep}: {reads} reads in {dt * 1e3:.1f} ms = {reads / dt / 1e6:.1f} M reads/s ({n / dt / 1e9:.2f} GB/s of gzip); repairs so far {ing.gzip_repairs()}", flush=True)
    print(f"best: {reads / best / 1e6:.1f} M reads/s (chunks of {chunk >> 20} MB, pieces of {os.environ.get('GMX_GZ_PIECE', '32768')} B)")


def gram(d, reps):
    from gramtools_amd.build import build_gram
    g = build_gram()
    for rep in range(reps):
        for name, env in (("device", {}), ("host", {"GMX_HOST_GZ": "1"})):
            e = dict(os.environ, **env)
            out = os.path.join(d, f"out_{name}_{rep}")
            t0 = time.perf_counter()
            r = subprocess.run([g, "genotype", "--gram_dir", d, "--reads", os.path.join(d, "r.fq.gz"), "--sample_id", "s", "--ploidy", "haploid",
                                "--kmer_size", "10", "--genotype_dir", out, "--seed", "42", "--max_threads", "1"],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=e)
            dt = time.perf_counter() - t0
            feed = [l.strip() for l in r.stdout.splitlines() if "Quasimap (" in l or "warning" in l]
            print(f"rep {rep} {name}: rc {r.returncode}, {dt:.2f} s wall; " + " | ".join(feed[-2:]), flush=True)
            if r.returncode:
                print(r.stdout[-2000:])
                return


def host(path, threads):
    from gramtools_amd.build import build_gram
    r = subprocess.run([build_gram(), "_parse_bench", path, str(threads), "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "make":
        make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4000000)
    elif mode == "chain":
        chain(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif mode == "gram":
        gram(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif mode == "host":
        host(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 16)

"""Quality trimming in the device's record scan (gmx_ingest_set_quality_trim, gmx_records_trim_kernel): the reads
an ingest hands over with trimming on are the reads cut in Python by the restated rule (tests/test_quality_trim_rule.py) — lengths,
planes, offsets, skip flags, the chunk's counters — through every submit call, and an ingest with trimming off is untouched."""
import gzip

import numpy as np
import pytest

from test_ingest import bgzf, check_reads, expected_planes, fastq
from test_quality_trim_rule import phred, trim_ref

pytestmark = pytest.mark.gpu

GMX_EINVAL = -1
Q = 20


# ---- reads with crafted quality strings ---------------------------------------------------------------------------------
def crafted_quals(rng, n):
    """Phred values for a read of n bases: one of the patterns of the rule's crafted cases, cut or padded to n."""
    kind = int(rng.integers(0, 9))
    good = [int(x) for x in rng.integers(30, 42, n)]
    if kind == 0:
        q = good                                                   # all high
    elif kind == 1:
        q = [int(x) for x in rng.integers(0, 15, n)]               # all low
    elif kind == 2:
        q = good[:-1] + [2]                                        # one low last base
    elif kind == 3:
        q = (good + [10, 25, 10])[-n:] if n >= 3 else good         # the running sum takes the good base in the tail too
    elif kind == 4:
        q = (good + [40, 10, 30, 10])[-n:] if n >= 4 else good     # a tie keeps the longer read
    elif kind == 5:
        q = [Q] * n                                                # q == Q removes nothing
    elif kind == 6:
        k = int(rng.integers(0, n + 1))                            # a poor tail of any length, the plane boundaries included
        q = good[:n - k] + [2] * k
    elif kind == 7:
        k = int(rng.integers(0, n + 1))                            # bytes below 33 count as quality 0 (-1: byte 32)
        q = good[:n - k] + [-1] * k
    else:
        q = [int(x) for x in rng.integers(0, 42, n)]               # anything
    return q[:n]


def trim_fastq(rng, n, lo, hi, crlf=False, final_newline=True, quals=None):
    """n records of lo..hi bases. Returns (text, sequences, quality strings as bytes). A third of the reads with a poor end hold an N
    there, every 11th read holds one anywhere."""
    nl = "\r\n" if crlf else "\n"
    seqs, quals_out, recs = [], [], []
    for i in range(n):
        ln = int(rng.integers(lo, hi + 1))
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, ln))
        q = bytes(33 + v for v in (quals(rng, ln) if quals else crafted_quals(rng, ln)))
        t = trim_ref(q, Q)
        if t < ln and i % 3 == 0:  # an N where the sequencer was unsure: in the part that goes (quality 2 in real files)
            k = int(rng.integers(t, ln))
            s = s[:k] + "N" + s[k + 1:]
        if i % 11 == 10:
            k = int(rng.integers(0, ln))
            s = s[:k] + "n" + s[k + 1:]
        seqs.append(s)
        quals_out.append(q)
        recs.append(f"@r{i} d:{i * 7919}{nl}{s}{nl}+{nl}".encode() + q + nl.encode())
    text = b"".join(recs)
    if not final_newline:
        text = text[:-len(nl)]
    return text, seqs, quals_out


def expected_stats(seqs, quals, q_min, m_min):
    ts = [trim_ref(q, q_min) for q in quals]
    return (sum(t < len(s) for s, t in zip(seqs, ts)), sum(len(s) - t for s, t in zip(seqs, ts)), sum(t < m_min for t in ts), sum(len(s) for s in seqs))


def check_trimmed(ing, slot, res, seqs, quals, q_min=Q, m_min=1):
    """What check_reads checks, on the reads cut in Python — and the skip rule of a trimming ingest: a letter other than ACGT within
    the bases kept, or fewer than m_min of them."""
    cut = [s[:trim_ref(q, q_min)] for s, q in zip(seqs, quals)]
    exp, offs, uniform = expected_planes(cut)
    assert res.status == 0, f"status {res.status} (member {res.bad_member})"
    assert res.n_reads == len(cut)
    assert res.uniform_len == uniform
    assert res.n_bases == int(offs[-1])
    ppr = (uniform + 31) // 32
    assert res.n_pairs == (len(cut) * ppr if uniform else (int(offs[-1]) >> 5) + len(cut))
    got = ing.fetch_reads(slot, res)
    letters_ok = np.array([set(s.upper()) <= set("ACGT") for s in cut])
    skip_exp = np.array([0 if ok and len(s) >= m_min else 1 for s, ok in zip(cut, letters_ok)], dtype=np.uint8)
    assert (got.skip[:len(cut)] == skip_exp).all(), np.nonzero(got.skip[:len(cut)] != skip_exp)[0][:10]
    assert bool(res.any_skip) == bool(skip_exp.any())
    if not uniform:
        assert (got.offsets == offs).all()
    for r, s in enumerate(cut):  # (a read with another letter: its planes are whatever the letter's bits give)
        if not letters_ok[r]:
            continue
        p0 = r * ppr if uniform else (int(offs[r]) >> 5) + r
        k = (len(s) + 31) // 32
        assert (got.planes[p0:p0 + k] == exp.planes[p0:p0 + k]).all(), f"read {r}"
    assert ing.trim_stats(slot) == expected_stats(seqs, quals, q_min, m_min)
    return cut


@pytest.fixture(scope="module")
def ing():
    from gramtools_amd import Ingest
    g = Ingest(max_text_bytes=1 << 20)
    yield g
    g.close()


@pytest.fixture(scope="module")
def mixed():
    """The file most tests share: 300 reads of 1..70 bases with every crafted quality pattern."""
    return trim_fastq(np.random.default_rng(70), 300, 1, 70)


def fresh(ing, q_min=Q, m_min=1):
    ing.reset()
    ing.set_format(0)
    ing.set_quality_trim(q_min, m_min)


# ---- the reads, one chunk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_min", [1, 20])
@pytest.mark.parametrize("crlf,final_newline", [(False, True), (True, True), (False, False), (True, False)])
def test_trimmed_reads_equal_the_reads_cut_in_python(ing, m_min, crlf, final_newline):
    """Lengths 1..70: trimmed ends on both sides of the 32- and 64-base plane boundaries; every quality pattern; Ns in the part that
    goes (not skipped) and in the part that stays (skipped); reads left shorter than min_length skipped; CRLF; no last newline."""
    text, seqs, quals = trim_fastq(np.random.default_rng(7 + m_min), 300, 1, 70, crlf=crlf, final_newline=final_newline)
    fresh(ing, Q, m_min)
    ing.submit_text(0, text, True)
    res = ing.wait(0)
    cut = check_trimmed(ing, 0, res, seqs, quals, Q, m_min)
    # the file has what the test is about
    ts = [len(c) for c in cut]
    assert {31, 32, 33} & set(ts) and {63, 64, 65} & set(ts) and 0 in ts
    assert any("N" in s[t:] and "N" not in s[:t] and "n" not in s[:t] and t >= m_min for s, t in zip(seqs, ts))
    assert res.tail_bytes == 0


@pytest.mark.parametrize("q_min", [1, 2, 30, 93])
def test_other_thresholds(ing, mixed, q_min):
    text, seqs, quals = mixed
    fresh(ing, q_min, 5)
    ing.submit_text(1, text, True)
    check_trimmed(ing, 1, ing.wait(1), seqs, quals, q_min, 5)


def test_uniform_in_ragged_out_and_back(ing):
    rng = np.random.default_rng(3)
    # one shortened read among reads of one length: the offsets form
    count = iter(range(200))
    text, seqs, quals = trim_fastq(rng, 200, 50, 50, quals=lambda r, n: [38] * 41 + [2] * 9 if next(count) == 77 else [38] * n)
    assert quals[77] == phred([38] * 41 + [2] * 9) and quals[78] == phred([38] * 50)
    fresh(ing)
    ing.submit_text(0, text, True)
    res = ing.wait(0)
    assert res.uniform_len == 0
    check_trimmed(ing, 0, res, seqs, quals)
    # every read trimmed to one length (from different lengths): uniform
    text, seqs, quals = trim_fastq(rng, 200, 40, 70, quals=lambda r, n: [38] * 33 + [2] * (n - 33))
    fresh(ing)
    ing.submit_text(1, text, True)
    res = ing.wait(1)
    assert res.uniform_len == 33
    check_trimmed(ing, 1, res, seqs, quals)
    # every read trimmed to nothing: reads of length 0, as FASTA's
    text, seqs, quals = trim_fastq(rng, 200, 1, 70, quals=lambda r, n: [2] * n)
    fresh(ing)
    ing.submit_text(0, text, True)
    res = ing.wait(0)
    assert res.uniform_len == 0 and res.n_pairs == res.n_reads == 200 and res.n_bases == 0
    check_trimmed(ing, 0, res, seqs, quals)


# ---- the same file through every submit call -------------------------------------------------------------------------------
def feed_and_check(submit, ing, seqs, quals, n_chunks, m_min=1):
    """Chunks 0 .. n_chunks - 1 through submit(slot, k), alternating slots; every chunk's reads and counters checked. Returns the reads seen."""
    got = 0
    for k in range(n_chunks):
        slot = k % 2
        submit(slot, k)
        res = ing.wait(slot)
        n = int(res.n_reads)
        if n:
            check_trimmed(ing, slot, res, seqs[got:got + n], quals[got:got + n], Q, m_min)
        else:
            assert res.status == 0 and ing.trim_stats(slot) == (0, 0, 0, 0)
        got += n
    return got


def test_text_cut_at_every_byte_of_one_record(ing):
    """Two chunks, the cut walking through one record — header, bases, '+', qualities, the line ends: the record's quality line is then
    in the carried text, in the new text, or across both."""
    text, seqs, quals = trim_fastq(np.random.default_rng(12), 40, 20, 70)
    rec_bytes = [len(f"@r{i} d:{i * 7919}\n{s}\n+\n") + len(s) + 1 for i, s in enumerate(seqs)]
    assert sum(rec_bytes) == len(text)
    start = sum(rec_bytes[:17])  # record 17 starts here
    for cut in range(start, start + rec_bytes[17] + 1):
        fresh(ing)
        parts = (text[:cut], text[cut:])
        got = feed_and_check(lambda slot, k: ing.submit_text(slot, parts[k], k == 1), ing, seqs, quals, 2)
        assert got == len(seqs), cut


def test_bgzf_and_gzip(ing, mixed, monkeypatch):
    from gramtools_amd import bgzf_members
    text, seqs, quals = mixed
    # BGZF: members of 1500 bytes, three chunks
    data = bgzf(text, block=1500)
    mem = bgzf_members(data)
    third = (len(mem) + 2) // 3
    chunks = [mem[i:i + third] for i in range(0, len(mem), third)]

    def submit_bgzf(slot, k):
        ch = chunks[k]
        lo, hi = ch[0][0], ch[-1][0] + ch[-1][1]
        ing.submit_bgzf(slot, data[lo:hi], [(o - lo, s, i, c) for o, s, i, c in ch], k == len(chunks) - 1)
    fresh(ing, Q, 20)
    assert feed_and_check(submit_bgzf, ing, seqs, quals, len(chunks), 20) == len(seqs)
    # plain gzip: pieces of 1 KB, two chunks with look-ahead
    monkeypatch.setenv("GMX_GZ_PIECE", "1024")
    gz = gzip.compress(text, 6)
    half = len(gz) // 2

    def submit_gzip(slot, k):
        if k == 0:
            ing.submit_gzip(slot, gz, half, False)
        else:
            ing.submit_gzip(slot, gz[half:], len(gz) - half, True)
    fresh(ing, Q, 20)
    assert feed_and_check(submit_gzip, ing, seqs, quals, 2, 20) == len(seqs)


@pytest.mark.parametrize("compressed", [False, True])
def test_chunks_dealt_over_two_ingests(ing, mixed, compressed):
    """The several-GPU form: chunks uploaded ahead (_deferred) on two ingests in turn, scanned in file order with the cut record
    handed over through the host."""
    from gramtools_amd import Ingest, bgzf_members
    text, seqs, quals = mixed
    other = Ingest(max_text_bytes=1 << 20)
    ings = [ing, other]
    for g in ings:
        fresh(g, Q, 20)
    if compressed:
        data = bgzf(text, block=2000)
        mem = bgzf_members(data)
        chunks = [mem[i:i + 2] for i in range(0, len(mem), 2)]
    else:
        chunks = [text[i:i + 3001] for i in range(0, len(text), 3001)]

    def submit(c):
        g, slot = ings[c % 2], (c // 2) & 1
        if compressed:
            ch = chunks[c]
            lo, hi = ch[0][0], ch[-1][0] + ch[-1][1]
            g.submit_bgzf_deferred(slot, data[lo:hi], [(o - lo, s, i, k) for o, s, i, k in ch])
        else:
            g.submit_text_deferred(slot, chunks[c])
    for c in range(min(len(chunks), 4)):
        submit(c)
    got, tail = 0, b""
    for c in range(len(chunks)):
        g, slot = ings[c % 2], (c // 2) & 1
        g.scan(slot, tail, c == len(chunks) - 1)
        res = g.wait(slot)
        n = int(res.n_reads)
        if n:
            check_trimmed(g, slot, res, seqs[got:got + n], quals[got:got + n], Q, 20)
        got += n
        tail = g.fetch_tail(slot)
        if c + 4 < len(chunks):
            submit(c + 4)
    assert got == len(seqs) and tail == b""
    other.close()


# ---- off means off ---------------------------------------------------------------------------------------------------------
def result_bytes(g, slot, res):
    got = g.fetch_reads(slot, res)
    fields = (res.status, res.n_reads, res.n_bases, res.n_pairs, res.uniform_len, res.any_skip, res.text_bytes, res.consumed_bytes, res.tail_bytes, tuple(res.sub_pairs))
    return fields, got.planes[:int(res.n_pairs)].tobytes(), None if got.offsets is None else got.offsets.tobytes(), got.skip.tobytes()


def test_threshold_0_is_an_ingest_on_which_the_call_was_never_made(ing, mixed):
    from gramtools_amd import Ingest
    text, seqs, quals = mixed
    never = Ingest(max_text_bytes=1 << 20)
    never.submit_text(0, text, True)
    res0 = never.wait(0)
    check_reads(never, 0, res0, seqs)
    assert never.trim_stats(0) == (0, 0, 0, 0)
    want = result_bytes(never, 0, res0)
    never.close()
    fresh(ing, Q, 20)  # on ...
    ing.submit_text(0, text, True)
    assert result_bytes(ing, 0, ing.wait(0)) != want
    fresh(ing, 0, 0)   # ... and off again (min_length is ignored)
    ing.submit_text(1, text, True)
    res = ing.wait(1)
    assert result_bytes(ing, 1, res) == want
    assert ing.trim_stats(1) == (0, 0, 0, 0)


def test_what_the_call_refuses(ing, mixed):
    from gramtools_amd import GmxError, GMX_INGEST_FORMAT_BAM, GMX_INGEST_FORMAT_FASTQ
    text, seqs, quals = mixed
    fresh(ing, Q, 7)

    def refused(call, *args):
        with pytest.raises(GmxError) as e:
            call(*args)
        assert e.value.code == GMX_EINVAL
    refused(ing.set_quality_trim, 94, 1)
    refused(ing.set_quality_trim, 20, 0)
    refused(ing.set_quality_trim, 1 << 31, 1)
    assert ing.lib.gmx_ingest_set_quality_trim(None, 20, 1) == GMX_EINVAL
    assert ing.lib.gmx_ingest_trim_stats(None, 0, None) == GMX_EINVAL
    refused(ing.trim_stats, 3)
    ing.set_quality_trim(93, 1)
    ing.set_quality_trim(1, 1 << 31)
    ing.set_quality_trim(Q, 7)
    # a chunk in flight: neither the setting nor the counters
    ing.submit_text(0, text, True)
    refused(ing.set_quality_trim, 30, 1)
    refused(ing.set_quality_trim, 0, 0)
    refused(ing.trim_stats, 0)
    check_trimmed(ing, 0, ing.wait(0), seqs, quals, Q, 7)  # (the refused calls changed nothing)
    # a deferred chunk counts as in flight
    ing.reset()
    ing.submit_text_deferred(1, text)
    refused(ing.set_quality_trim, 30, 1)
    ing.scan(1, b"", True)
    check_trimmed(ing, 1, ing.wait(1), seqs, quals, Q, 7)
    # BAM, in either order
    refused(ing.set_format, GMX_INGEST_FORMAT_BAM)
    ing.set_quality_trim(0, 0)
    ing.set_format(GMX_INGEST_FORMAT_BAM)
    refused(ing.set_quality_trim, Q, 1)
    ing.set_quality_trim(0, 5)  # (off is accepted in every format)
    ing.set_format(GMX_INGEST_FORMAT_FASTQ)


@pytest.mark.parametrize("fmt", ["fasta", "lines"])
def test_formats_without_qualities_are_not_changed(ing, fmt):
    from gramtools_amd import GMX_INGEST_FORMAT_FASTA, GMX_INGEST_FORMAT_LINES, GMX_INGEST_FORMAT_FASTQ
    rng = np.random.default_rng(9)
    _, seqs = fastq(rng, 300, 1, 70, bad_every=13)
    if fmt == "fasta":
        text = "".join(f">r{i}\n{s[:30]}\n{s[30:]}\n" if len(s) > 30 else f">r{i}\n{s}\n" for i, s in enumerate(seqs)).encode()
    else:
        text = "".join(s + "\n" for s in seqs).encode()
    ing.reset()
    ing.set_quality_trim(0, 0)
    ing.set_format(GMX_INGEST_FORMAT_FASTA if fmt == "fasta" else GMX_INGEST_FORMAT_LINES)
    ing.submit_text(0, text, True)
    res = ing.wait(0)
    check_reads(ing, 0, res, seqs)
    want = result_bytes(ing, 0, res)
    ing.reset()
    ing.set_quality_trim(Q, 20)
    ing.submit_text(1, text, True)
    res = ing.wait(1)
    check_reads(ing, 1, res, seqs)
    assert result_bytes(ing, 1, res) == want
    assert ing.trim_stats(1) == (0, 0, 0, 0)
    ing.set_quality_trim(0, 0)
    ing.set_format(GMX_INGEST_FORMAT_FASTQ)

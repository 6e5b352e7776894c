"""The crafted deflate streams of tests/test_inflate_crafted.py (device) and tests/test_deflate_craft_host.py (zlib, no GPU):
module-level lists, built once with tests/deflate_craft.py. VALID streams inflate to expand(tokens); INVALID ones are refused by
zlib, and each names the test in gmx_ingest.hip that refuses it on the device (read before the stream first ran there)."""
import zlib

import numpy as np

from deflate_craft import (Deflate, Match, RawLL, expand, limited_lengths, kraft, LENGTH_BASE, LENGTH_EXTRA, DIST_BASE, DIST_EXTRA,
                           gzip_member, greedy_cl_ops, GZ_HDR)

PRINTABLE = list(range(0x20, 0x7F)) + [10]
BINARY = list(range(0, 9)) + list(range(14, 32)) + list(range(127, 256))


class Case:
    """One deflate stream. text: what it inflates to (valid), or only a length for the member's ISIZE (invalid). trunc: the
    damage is a truncation (zlib is left incomplete, it does not raise). crc / isize: a wrong trailer. tail: bytes behind the
    deflate data inside the member. gz_prefix: a whole valid gzip member that stands in front (gzip route). guard: where
    gmx_ingest.hip refuses it."""

    def __init__(self, name, deflate, text, valid=True, routes=("bgzf", "gzip"), trunc=False, crc=None, isize=None, tail=b"", gz_prefix=b"",
                 guard="", big=None):
        self.name, self.deflate, self.text, self.valid, self.routes = name, deflate, text, valid, routes
        self.trunc, self.crc, self.isize, self.tail, self.gz_prefix, self.guard = trunc, crc, isize, tail, gz_prefix, guard
        self.big = len(deflate) >= 2048 if big is None else big

    def __repr__(self):
        return self.name


def of(name, d, **kw):
    return Case(name, d.getvalue(), d.text(), **kw)


def rnd(seed, n, alphabet=None):
    rng = np.random.default_rng(seed)
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return bytes(np.array(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


def lens_of(n, assign):
    lens = [0] * n
    for s, l in assign.items():
        lens[s] = l
    return lens


SKEW = list(range(1, 15)) + [15, 15]  # the most skewed complete code: 1, 2, ..., 14, 15, 15


def mixed(syms, seed, times=3):
    rng = np.random.default_rng(seed)
    seq = list(syms) * times
    rng.shuffle(seq)
    return seq


# ------------------------------------------------------------------------------------------------------------------
# code shapes
# ------------------------------------------------------------------------------------------------------------------
def code_shape_cases():
    out = []
    # literal/length codes of every length 1..15; the 10- and 11-bit symbols are the two sides of ING_LIT_ROOT
    lits = list(b"etaoinshrdlucm")
    variants = {
        "lit15_literal_eob": lits[:13] + [258, ord("Z"), 256],            # 15 bits: a literal and the end of the block
        "lit15_eob_length": lits[:13] + [ord("Z"), 256, 260],             # 15 bits: the end of the block and a length
        "lit15_literal_length": [256] + lits[:8] + [264, 270] + lits[8:11] + [ord("Z"), 285],  # lengths at 10, 11 and 15 bits
    }
    for name, order in variants.items():
        ll = lens_of(286, dict(zip(order, SKEW)))
        toks = [s for s in order if s < 256] * 2
        for s in mixed([s for s in order if s != 256], len(name)):
            if s < 256:
                toks.append(s)
            else:
                i = s - 257
                toks.append(Match(LENGTH_BASE[i] + ((1 << LENGTH_EXTRA[i]) - 1), 1 + len(toks) % 7, lsym=s))
                toks.append(Match(LENGTH_BASE[i], 2, lsym=s))
        out.append(of(name, Deflate().dynamic(toks, True, lit_lens=ll)))
    # the same for the distance code: 7 and 8 bits around ING_DIST_ROOT, symbols 28 and 29 at 15 bits
    front = rnd(1, 32768)
    dorder = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 28, 29]
    dl = lens_of(30, dict(zip(dorder, SKEW)))
    toks = []
    for s in mixed(dorder, 2):
        toks += [Match(3 + s, DIST_BASE[s]), ord("x"), Match(9, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)]
    out.append(of("dist_every_length_1_to_15", Deflate().stored(front).dynamic(toks, True, dist_lens=dl)))
    # the widest token: 15-bit code of 284 + 5 extra bits, 15-bit distance code + 13 extra bits, at every bit phase 0..31 of the
    # stream (each round below is 49 bits, 49 and 32 are coprime), directly after a literal and several in a row
    ll = lens_of(286, dict(zip(list(b"abcdefghijklmn") + [284, 256], SKEW)))
    dl = lens_of(30, dict(zip(list(range(14)) + [28, 29], SKEW)))
    d = Deflate().stored(front)
    toks = []
    for k in range(36):
        toks += [ord("a"), Match(227 + (k * 7) % 32, (24577 if k % 2 else 16385) + (8191 if k % 5 == 0 else (k * 997) % 8192), lsym=284)]
    toks += [Match(258, 32768, lsym=284), Match(227, 24577), Match(257, 16385 + 8191)]
    d.dynamic(toks, True, lit_lens=ll, dist_lens=dl)
    out.append(of("widest_token_every_bit_phase", d))
    # every length 3..258 and both ends (and the middle) of every distance symbol's range; 258 as 285 and as 284 + 31
    for name, lo, hi in (("lengths_3_130_all_distance_symbols", 3, 130), ("lengths_131_258", 131, 258)):
        toks = []
        for ln in range(lo, hi + 1):
            toks += [Match(ln, 1 + (ln * 37) % 300), ln & 0xFF]
        if lo == 3:
            for s in range(30):
                span = 1 << DIST_EXTRA[s]
                for dist in sorted({DIST_BASE[s], DIST_BASE[s] + span // 2, DIST_BASE[s] + span - 1}):
                    toks += [Match(3 + s % 5, dist), s]
        else:
            toks += [Match(258, 9), Match(258, 9, lsym=284), Match(258, 5000, lsym=284), Match(258, 5000)]
        for i in range(29):  # every length symbol at extra 0 and at its maximum
            toks += [Match(LENGTH_BASE[i], 40, lsym=257 + i), Match(LENGTH_BASE[i] + (1 << LENGTH_EXTRA[i]) - 1, 40, lsym=257 + i)]
        out.append(of(name, Deflate().stored(front).dynamic(toks, True)))
        if lo == 3:
            out.append(of(name + "_fixed", Deflate().stored(front).fixed(toks, True)))
    # all 286 literal/length and all 30 distance symbols in one block (HLIT 286, HDIST 30), and the minima (HLIT 257, HDIST 1)
    toks = list(range(256))
    for i in range(29):
        toks += [Match(LENGTH_BASE[i], DIST_BASE[i], lsym=257 + i), i]
    toks += [Match(4, DIST_BASE[29])]
    d = Deflate().stored(front).dynamic(toks, True)
    out.append(of("hlit_286_hdist_30", d))
    d = Deflate().dynamic(list(b"only literals, the smallest header"), True, dist_lens=[0])
    out.append(of("hlit_257_hdist_1_no_distance_code", d))
    # one distance code of length 1 (RFC 1951 §3.2.7: incomplete and valid)
    out.append(of("one_distance_code", Deflate().dynamic(list(b"abc") + [Match(3, 1), ord("d"), Match(258, 1), Match(17, 1)], True, dist_lens=[1])))
    # one literal and the end of the block, one bit each
    out.append(of("one_literal_and_eob", Deflate().dynamic([ord("A")] * 777, True, lit_lens=lens_of(257, {65: 1, 256: 1}), dist_lens=[0])))
    return out


def empty_block_cases():
    out = []
    text = rnd(3, 300, PRINTABLE)
    kinds = {
        "dynamic": lambda d, f: d.dynamic([], f, lit_lens=lens_of(257, {256: 1}), dist_lens=[0]),  # only the end-of-block code
        "fixed": lambda d, f: d.fixed([], f),
        "stored": lambda d, f: d.stored(b"", f),
    }
    for name, put in kinds.items():
        d = Deflate()
        put(d, False)
        d.fixed(list(text[:150]))
        for _ in range(5):
            put(d, False)
        d.dynamic(list(text[150:]) + [Match(20, 150)])
        put(d, True)
        out.append(of(f"empty_{name}_blocks_first_between_last", d))
        d = Deflate()
        put(d, True)
        out.append(of(f"only_an_empty_{name}_block", d))
    d = Deflate()
    for k in range(9):
        kinds[("dynamic", "fixed", "stored")[k % 3]](d, False)
    d.fixed(list(text), True)
    out.append(of("empty_blocks_of_every_kind_in_a_row", d))
    # zlib itself, flushed every 1000 bytes (what pigz does every 128 KB): an empty stored block per flush
    fq = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, rnd(i, 60, list(b"ACGT")), rnd(i + 900, 60, list(range(35, 74)))) for i in range(40))
    for name, mode in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH)):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = b"".join(c.compress(fq[i:i + 1000]) + c.flush(mode) for i in range(0, len(fq), 1000)) + c.flush()
        out.append(Case(f"zlib_{name}_flush_every_1000", body, fq))
    return out


def header_cases():
    """The code-length header (§3.2.7)."""
    out = []
    # HCLEN 5 (16 17 18 0 8): every code has 8 bits. (HCLEN 4 can only send zeros: no end-of-block code, see INVALID.)
    ll = [8] * 255 + [0, 8]
    out.append(of("hclen_5", Deflate().dynamic(list(range(0, 255, 3)), True, lit_lens=ll, dist_lens=[0], hclen=5)))
    # HCLEN 19 with a code-length code of 1..7 bits (eight symbols: 18, 0, 1..6)
    cl = lens_of(19, {18: 1, 0: 2, 1: 3, 2: 4, 3: 5, 4: 6, 5: 7, 6: 7})
    ll7 = lens_of(257, {97: 1, 98: 2, 99: 3, 100: 4, 101: 5, 102: 6, 256: 6})
    ops = [(18, 97), 1, 2, 3, 4, 5, 6, (18, 138), (18, 14), 0, 6, 0]
    out.append(of("hclen_19_code_length_codes_of_7_bits", Deflate().dynamic(list(b"abcdefabcaba" * 5), True, lit_lens=ll7, dist_lens=[0], cl_lens=cl, cl_ops=ops,
                                                                       hclen=19)))
    # HCLEN 19 with every length 1..15 (15 is the last of the order)
    ll = lens_of(286, dict(zip(list(b"abcdefghijklmn") + [285, 256], SKEW)))
    out.append(of("hclen_19_lengths_1_to_15", Deflate().dynamic(list(b"abcdefghijklmn") + [Match(258, 2)], True, lit_lens=ll, hclen=19)))
    # every repeat count: 16 at 3..6, 17 at 3..10, 18 at 11..138 (the first run that can hold the repeat starts with it)
    d = Deflate()
    body = list(b"abcdefg" * 3)
    for rep in range(3, 7):    # a run of seven 3s: literals a..g, the eighth code is the end of the block
        d.dynamic(body, False, lit_lens=lens_of(257, dict([(s, 3) for s in b"abcdefg"] + [(256, 3)])), dist_lens=[0], force=(16, rep))
    for rep in range(3, 11):
        d.dynamic(body, False, lit_lens=lens_of(257, dict([(s, 3) for s in b"abcdefg"] + [(256, 3)])), dist_lens=[0], force=(17, rep))
    out.append(of("repeat_16_at_3_to_6_and_17_at_3_to_10", d.fixed([], True)))
    d = Deflate()
    for rep in range(11, 139):
        first = 10 + rep  # symbols 6 .. 9 + rep have no code: a zero run of rep + 4, which the forced (18, rep) opens
        ll = lens_of(257, {5: 2, first: 2, first + 1: 2, 256: 2})
        d.dynamic([5, first, first + 1, 5], False, lit_lens=ll, dist_lens=[0], force=(18, rep))
    out.append(of("repeat_18_at_11_to_138", d.fixed([], True)))
    # a 16 run and an 18 run that begin in the literal lengths and end in the distance lengths
    ll = lens_of(259, {ord("a"): 2, ord("b"): 2, 256: 3, 257: 3, 258: 2})
    ll[256], ll[257], ll[258] = 3, 3, 3  # a 2, b 2, 256 / 257 / 258 3: Kraft 1/4 + 1/4 + 3/8 = 7/8 -> one more 3
    ll[ord("c")] = 3
    dl = [3] * 8
    ops = [(18, 97), 2, 2, 3, (18, 138), (18, 256 - 100 - 138), 3, 3, (16, 6), 3, 3, 3]  # the 16: symbol 258 and distance symbols 0..4
    toks = list(b"abcab") + [Match(3, 1), Match(4, 2), Match(3, 8), Match(3, 5)]
    out.append(of("repeat_16_across_hlit", Deflate().dynamic(toks, True, lit_lens=ll, dist_lens=dl, cl_ops=ops)))
    ll = lens_of(286, {ord("a"): 2, ord("b"): 2, 256: 2, 257: 2})
    dl = [0] * 20 + [1, 1]
    ops = [(18, 97), 2, 2, (18, 138), (18, 256 - 99 - 138), 2, 2, (18, 28 + 20), 1, 1]  # the last 18: symbols 258..285 and distance symbols 0..19
    toks = list(b"ab" * 1000) + [Match(3, 1025), Match(3, 1537)]
    out.append(of("repeat_18_across_hlit", Deflate().dynamic(toks, True, lit_lens=ll, dist_lens=dl, cl_ops=ops)))
    # 16 directly after 17 and after 18: it repeats the zero
    ll = lens_of(257, {40: 2, 41: 2, 200: 2, 256: 2})
    ops = [(17, 10), (16, 6), (18, 21), (16, 3), 2, 2, (18, 138), (16, 6), (18, 14), 2, (18, 55), 2, 0]
    out.append(of("repeat_16_after_17_and_18", Deflate().dynamic([40, 41, 200, 41], True, lit_lens=ll, dist_lens=[0], cl_ops=ops)))
    return out


def fused_literal_cases():
    """ing_fuse: two and three literals in one table entry; a third literal >= 128 is not fused (bit 31 is ING_RARE)."""
    out = []
    # 2- and 3-bit codes for byte values below and above 128; all 64 triples of them: every pattern of high / low
    ll = lens_of(258, {0x41: 2, 0xC1: 2, 0x42: 3, 0xC2: 3, 256: 3, 257: 4, 0x43: 5, 0xC3: 5})
    four = [0x41, 0xC1, 0x42, 0xC2]
    toks = [a for x in four for y in four for z in four for a in (x, y, z)]
    toks += [0x43, 0xC3, 0x43, 0x43, 0xC3, 0xC3]
    for x in four:  # a literal directly followed by a length code that shares its root entry, and by the end of the block
        toks += [x, Match(3, 1)]
    toks += [0xC1]
    out.append(of("fused_literals_high_and_low", Deflate().dynamic(toks, True, lit_lens=ll, dist_lens=[1])))
    # code lengths 2 2 3 3 4 5 6 6 (+ end of block 4, length 257 4): all 512 triples — pairs of 10 and 11 bits (5+5, 4+6, 5+6),
    # triples of exactly 10 (2+3+5, 3+3+4, 2+2+6) and of 11
    ll = lens_of(258, {0x30: 2, 0xB0: 2, 0x31: 3, 0xB1: 3, 0x32: 4, 0xB5: 5, 0x36: 6, 0xB6: 6, 256: 4, 257: 4})
    assert kraft(ll) == 1 << 15
    eight = [0x30, 0xB0, 0x31, 0xB1, 0x32, 0xB5, 0x36, 0xB6]
    toks = [a for x in eight for y in eight for z in eight for a in (x, y, z)]
    for x in eight:
        toks += [x, Match(3, 2), x]
    out.append(of("fused_literals_sums_10_and_11", Deflate().dynamic(toks, False, lit_lens=ll, dist_lens=[1, 1]).dynamic([0x30], True, lit_lens=ll, dist_lens=[0])))
    return out


# ------------------------------------------------------------------------------------------------------------------
# copies
# ------------------------------------------------------------------------------------------------------------------
COPY_LENS = (3, 4, 63, 64, 65, 127, 128, 129, 257, 258)


def copy_cases():
    out = []
    for lo, hi in ((1, 24), (25, 48), (49, 70)):  # every distance 1..70 with every length: dist == len, len +- 1, no divisor of 64
        toks = list(rnd(lo, 70))
        for dist in range(lo, hi + 1):
            for ln in COPY_LENS:
                toks += [Match(ln, dist), (dist * 7 + ln) & 0xFF]
        out.append(of(f"overlapping_copies_dist_{lo}_{hi}", Deflate().dynamic(toks, True)))
    # distances around the window thresholds of both routes (ING_NEAR_MAX 1728, GZ_NEAR_MAX 704, the rings 2048 / 1024), and the format's end
    front = rnd(7, 32768)
    toks = []
    for dist in (703, 704, 705, 1023, 1024, 1025, 1727, 1728, 1729, 2047, 2048, 2049, 32767, 32768):
        toks += [Match(3, dist), dist & 0xFF, Match(258, dist), (dist >> 8) & 0xFF]
    out.append(of("distances_around_the_window_thresholds", Deflate().stored(front).dynamic(toks, False).fixed(toks, True)))
    # a match whose target is the member's last 258 bytes
    out.append(of("match_is_the_last_258_bytes", Deflate().fixed(list(rnd(8, 500)) + [Match(258, 300)], True)))
    return out


def straddle_cases():
    """A 258-byte match that begins at output position p: around the flushes (1024 bytes in the BGZF route, 256 symbols in the gzip
    route). The texts are multiples of 1024 bytes, so that with many of them in a row (one BGZF submit, one gzip file) every
    member starts on such a boundary and p is the decoder's own position modulo the flush. The far match with the least room: dist = threshold + 1, len 258, from the last byte before a
    flush (a far source that ends AT the last flushed byte does not exist: dist would be at most 1023 + 258 < 1729)."""
    out = []
    for p in (255, 256, 257, 511, 1023, 1024, 1025, 2047, 2048, 2049, 3071):
        for dist in (1, 100, 255, 705, 1729):
            if dist > p:
                continue
            toks = list(rnd(p * 3 + dist, p)) + [Match(258, dist)]
            toks += list(rnd(5, (-len(expand(toks))) % 1024))
            out.append(of(f"match_258_at_{p}_dist_{dist}", Deflate().dynamic(toks, True), big=False))
    return out


def stored_cases():
    out = []
    d = Deflate()
    for i, ln in enumerate((1, 63, 64, 65, 1023, 1024, 1025)):  # stored after stored
        d.stored(rnd(20 + i, ln))
    out.append(of("stored_blocks_of_every_length", d.stored(rnd(30, 7), True)))
    out.append(of("stored_65535", Deflate().stored(rnd(31, 65535)).fixed(list(b"tail"), True), routes=("gzip",)))
    # the block in front ends at each of the eight bit offsets: empty fixed blocks (10 bits), one literal of 9 bits for the odd ones
    seen = set()
    for odd in (0, 1):
        for k in range(4):
            d = Deflate()
            if odd:
                d.fixed([200])
            for _ in range(k):
                d.fixed([])
            seen.add(d.bit_pos() % 8)
            name = f"stored_after_bit_offset_{d.bit_pos() % 8}"
            d.stored(rnd(40 + k, 100)).fixed(list(b"and on"), True)
            out.append(of(name, d))
    assert seen == set(range(8)), seen
    # stored data followed directly by a dynamic block
    d = Deflate().stored(rnd(50, 333)).dynamic(list(rnd(51, 200, PRINTABLE)) + [Match(100, 333)], True)
    out.append(of("stored_then_dynamic", d))
    return out


# ------------------------------------------------------------------------------------------------------------------
# gzip route: references into the bytes in front of a piece (GMX_GZ_PIECE 1024)
# ------------------------------------------------------------------------------------------------------------------
FRONT_PIECE = 1024
FRONT_DISTS = (1, 704, 705, 1024, 1025, 32768)


def piece_front_stream(printable):
    """(gzip file, text, cuts): one member whose blocks start exactly where the decoder's pieces start (checked below by the
    rule of gmx_gz_link_kernel: a piece starts where the one before ended, and ends with the first block that ends at or beyond the
    next piece's nominal start). Every such block begins with a match into the text in front of it."""
    alpha = PRINTABLE if printable else BINARY
    seed = 100 if printable else 200
    d = Deflate()
    d.stored(rnd(seed, 33877, alpha))  # ends at byte 10 + 5 + 33877 of the file: inside piece 33
    firsts = []

    def block(first_tokens, k):
        firsts.append(len(d.block_bits) - 1)
        d.dynamic(list(first_tokens) + list(rnd(seed + k, 1500, alpha[:64])), False)

    k = 0
    for dist in FRONT_DISTS:  # the first token of the piece's first block reaches `dist` back
        k += 1
        block([Match(258, dist), alpha[k], Match(3, dist)], k)
    k += 1
    block(list(rnd(seed + 50, 100, alpha)) + [Match(200, 250)], k)  # the source starts in front of the piece and ends inside it
    k += 1
    block([Match(258, 100)], k)                                      # ... and overlaps what it writes (dist < len)
    # a byte from 32 768 back, copied again by the first match of the next piece, and of the one after, and of a fourth
    prev = None
    for _ in range(4):
        k += 1
        n0 = len(d.text())
        block([Match(10, 32768 if prev is None else prev)], k)
        prev = len(d.text()) - n0
    chain_first = firsts[-4]
    d.fixed(list(rnd(seed + 60, 20, alpha)), True)
    text = d.text()
    bits = [b + 80 for b in d.block_bits]  # within the file: the 10-byte header in front
    # the pieces, by the decoder's rule
    starts, at, n_pieces = set(), bits[0], (len(d.getvalue()) + 18 + FRONT_PIECE - 1) // FRONT_PIECE
    ends = bits[1:]
    for i in range(n_pieces):
        stop = (i + 1) * FRONT_PIECE * 8
        if i and at >= stop:
            continue
        starts.add(at)
        nxt = [e for e in ends if e > at and e >= stop]
        if not nxt:
            break
        at = nxt[0]
    for b in firsts:
        assert bits[b] in starts, (b, bits[b])
    cuts = [bits[chain_first] // 8, bits[chain_first + 1] // 8]  # chunk cuts between a source and its reference
    return gzip_member(d.getvalue(), text), text, cuts


# ------------------------------------------------------------------------------------------------------------------
# seeded random differential
# ------------------------------------------------------------------------------------------------------------------
RANDOM_SEED = 20261018


def deepen(lens, rng, steps):
    """Lengthen random codes toward 15 bits; the Kraft sum stays what it was (a code of l bits and an unused symbol become two
    codes of l + 1 bits)."""
    lens = list(lens)
    for _ in range(steps):
        used = [s for s, l in enumerate(lens) if 0 < l < 15]
        free = [s for s, l in enumerate(lens) if l == 0]
        if not used or not free:
            break
        s, u = used[int(rng.integers(len(used)))], free[int(rng.integers(len(free)))]
        lens[s] += 1
        lens[u] = lens[s]
    return lens


def random_blocks(rng, target):
    """Block specifications [(kind, tokens, keyword arguments)] of one stream of about `target` bytes of text."""
    blocks, text_len, hist = [], 0, 0
    n_blocks = int(rng.integers(1, 5))
    for b in range(n_blocks):
        want = max(8, target // n_blocks)
        kind = ("stored", "fixed", "dynamic", "dynamic", "dynamic")[int(rng.integers(5))]
        if kind == "stored":
            data = rnd(int(rng.integers(1 << 30)), want)
            blocks.append(("stored", list(data), {}))
            text_len += want
            continue
        n_alpha = int(rng.choice([2, 4, 20, 90, 256]))
        alpha = rng.permutation(256)[:n_alpha]
        p_match = float(rng.choice([0.0, 0.1, 0.4, 0.8]))
        toks, made = [], 0
        while made < want:
            if text_len + made > 0 and want - made >= 3 and rng.random() < p_match:
                ln = min(want - made, int(rng.choice([3, 4, 5, 10, 64, 258, int(rng.integers(3, 259))])))
                dist = int(min(text_len + made, rng.choice([1, 2, 3, int(rng.integers(1, 40)), int(rng.integers(1, 2100)), int(rng.integers(1, 32769))])))
                toks.append(Match(ln, dist))
                made += ln
            else:
                toks.append(int(alpha[int(rng.integers(n_alpha))]))
                made += 1
        kw = {}
        if kind == "dynamic":
            fl, fd = Deflate.used_symbols(toks)
            noise = rng.random(286) ** 4 * float(rng.choice([0.0, 1.0, 30.0]))  # random frequencies: codes for unused symbols too
            ll = limited_lengths([f + (n if rng.random() < 0.5 else 0) for f, n in zip(fl, noise)], 15)
            dl = limited_lengths([f + (rng.random() if rng.random() < 0.3 else 0) for f in fd], 15)
            if sum(1 for l in ll if l) > 1:
                ll = deepen(ll, rng, int(rng.choice([0, 3, 40])))
            if sum(1 for l in dl if l) > 1:
                dl = deepen(dl, rng, int(rng.choice([0, 2, 10])))
            while len(ll) > 257 and ll[-1] == 0 and rng.random() < 0.8:
                ll.pop()
            while len(dl) > 1 and dl[-1] == 0 and rng.random() < 0.8:
                dl.pop()
            kw = {"lit_lens": ll, "dist_lens": dl}
            if rng.random() < 0.3:  # a code-length header without repeats, or with zero runs only
                lens = ll + dl
                if rng.random() < 0.5:
                    kw["cl_ops"] = lens
                kw["hclen"] = 19 if rng.random() < 0.5 else None
        blocks.append((kind, toks, kw))
        text_len += made
    return blocks


def render(blocks, final=True):
    d = Deflate()
    for i, (kind, toks, kw) in enumerate(blocks):
        last = final and i == len(blocks) - 1
        if kind == "stored":
            d.stored(bytes(toks), last)
        elif kind == "fixed":
            d.fixed(toks, last)
        else:
            d.dynamic(toks, last, **kw)
    return d


def random_specs(n=300):
    rng = np.random.default_rng(RANDOM_SEED)
    return [random_blocks(rng, int(rng.integers(512, 8193))) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------
# damage
# ------------------------------------------------------------------------------------------------------------------
def invalid_cases():
    out = []

    def bad(name, deflate, guard, n_text=100, **kw):
        out.append(Case(name, deflate, b"\0" * n_text, valid=False, guard=guard, **kw))

    some = list(b"some text to carry, some text to carry")
    good = Deflate().dynamic(some + [Match(20, 10)], True)
    w = Deflate()
    w.bits(1, 1)
    w.bits(3, 2)
    bad("btype_3", w.getvalue() + b"\0\0\0", "ing_inflate_member / gz_decode: `btype == 3`")
    bad("stored_nlen_mismatch", Deflate().stored(b"abcdef", True, nlen=0x1234).getvalue(), "`(len ^ nlen) != 0xFFFFu`", 6)
    bad("stored_len_beyond_the_member", Deflate().stored(b"abcdef", True, length=600).getvalue(),
        "`from + len > in_off + in_len` (BGZF), `from + len > nb` (gzip)", 600, trunc=True)  # (to zlib: data still to come)
    bad("hlit_287", Deflate().dynamic(some, True, hlit=287, invalid=True).getvalue(), "ing_block_tables: `hlit > 286u || hdist > 30u`")
    bad("hdist_31", Deflate().dynamic(some, True, hdist=31, invalid=True).getvalue(), "ing_block_tables: `hlit > 286u || hdist > 30u`")
    bad("hclen_4_only_zeros", Deflate().dynamic([], True, lit_lens=[0] * 257, dist_lens=[0], cl_lens=lens_of(19, {18: 1, 17: 1}), hclen=4, invalid=True,
                                                eob=False).getvalue(), "ing_block_tables: `L.lens[256] == 0` (HCLEN 4 can only send zeros)", 0)
    over = lens_of(257, {97: 1, 98: 1, 256: 1})
    bad("oversubscribed_literal_lengths", Deflate().dynamic([97, 98], True, lit_lens=over, dist_lens=[0], invalid=True).getvalue(),
        "ing_build: `left < 0`", 2)
    bad("oversubscribed_distances", Deflate().dynamic(some + [Match(3, 1)], True, dist_lens=[1, 1, 1], invalid=True).getvalue(), "ing_build: `left < 0`")
    bad("oversubscribed_code_length_code", Deflate().dynamic(some, True, cl_lens=lens_of(19, {0: 1, 3: 1, 4: 1, 5: 2, 18: 2, 17: 2, 6: 3}), invalid=True,
                                                             lit_lens=lens_of(257, dict([(s, 4) for s in set(some)] + [(256, 3)]))).getvalue(), "ing_build (kind 2): `left < 0`")
    ll = lens_of(257, {97: 1, 256: 1})
    bad("16_as_the_first_code_length_symbol", Deflate().dynamic([97], True, lit_lens=ll, dist_lens=[0], cl_ops=[(16, 3)] + greedy_tail(ll + [0], 3),
                                                                invalid=True).getvalue(), "ing_block_tables: `sym == 16u` with `at == 0`", 1)
    bad("repeat_past_hlit_plus_hdist", Deflate().dynamic([97], True, lit_lens=ll, dist_lens=[0], cl_ops=[(18, 97), 1, (18, 138), (17, 10), (17, 10), 1, (17, 3)],
                                                         invalid=True).getvalue(), "ing_block_tables: `at + rep > total`", 1)
    noeob = lens_of(257, {97: 1, 98: 1})
    bad("no_end_of_block_code", Deflate().dynamic([97, 98, 97], True, lit_lens=noeob, dist_lens=[0], invalid=True, eob=False).getvalue(),
        "ing_block_tables: `L.lens[256] == 0`", 3)
    # the unused code word of an incomplete set in the data: a single distance code (0) and the bit 1; a single literal/length code
    bad("unused_distance_code_word", unused_word(True), "ing_rare: `(e & 15u) == 0` (a table entry without a code)", 7)
    bad("unused_literal_code_word", unused_word(False), "ing_rare: `(e & 15u) == 0` (a table entry without a code)", 7)
    for sym in (286, 287):
        bad(f"fixed_literal_length_symbol_{sym}", Deflate().fixed(some + [RawLL(sym)] + some, True).getvalue(),
            "ing_entry: `s > 285u` gives ING_RARE without a length -> ing_rare: `(e & 15u) == 0`")
    for sym in (30, 31):
        bad(f"fixed_distance_symbol_{sym}", Deflate().fixed(some + [Match(3, None, dsym=sym)] + some, True).getvalue(),
            "ing_dist_entry: `s > 29u` gives ING_RARE without a length -> ing_rare: `(e & 15u) == 0`")
    # a distance one byte beyond the member's start (32 767 is the last position at which the format can say so)
    for at in (0, 5, 32767):
        d = Deflate()
        if at == 32767:
            d.stored(rnd(60, 32760))
        toks = list(rnd(61, at - len(d.tokens), PRINTABLE)) + [Match(3, at + 1)] + some
        bad(f"distance_beyond_the_start_at_{at}", d.fixed(toks, True).getvalue(),
            "the sign test `(out_pos - mis - dist) | ...` (BGZF), `(int)(out_pos - dist) < mstart` (gzip; from a later piece gmx_gz_link_kernel: `d.need > open`)",
            at + 3 + len(some))
    first = Deflate().fixed(list(b"a first member, complete\n"), True)
    # ... and the same beyond the start of a SECOND member, from a later piece: the text in front is the first member's, not zeros
    bad("distance_beyond_the_second_members_start_at_32767", out[-1].deflate,
        "gmx_gz_link_kernel: `d.need > open` (`open` starts again at a member's end: GzPiece::tail)", 32767 + 3 + len(some), routes=("gzip",),
        gz_prefix=gzip_member(Deflate().stored(rnd(63, 40000)).fixed(some, True).getvalue(), rnd(63, 40000) + bytes(some)))
    bad("second_member_inside_a_piece_starts_with_a_match", Deflate().fixed([Match(3, 1)] + some, True).getvalue(),
        "gz_decode: `mstart = (int)out_pos` at a member's start, then `(int)(out_pos - dist) < mstart`", routes=("gzip",),
        gz_prefix=gzip_member(first.getvalue(), first.text()))
    # the trailer and the member's size
    body, text = good.getvalue(), good.text()
    out.append(Case("isize_one_more", body, text, valid=False, isize=len(text) + 1,
                    guard="`out_pos != end_v` (BGZF: the last symbol's room test fails first), gmx_gz_check_kernel: `len != pc.end_isize[k]`"))
    out.append(Case("isize_one_less", body, text, valid=False, isize=len(text) - 1, guard="`out_pos + n_lit > end_v` / the sign test; gmx_gz_check_kernel"))
    out.append(Case("one_unused_byte_behind_the_deflate_data", body, text, valid=False, tail=b"\0", routes=("bgzf",),
                    guard="ing_inflate_member: `(used_bits + 7u) / 8u != in_len`"))
    # truncations: inside the dynamic header, inside a code, inside a stored block's data
    bad("truncated_in_the_dynamic_header", body[:6], "Bits::limit (zeros behind the member) -> the header's tests, or `used_bits`; gzip: `pos > nb * 8u`", trunc=True)
    bad("truncated_in_a_code", body[:len(body) - 3], "Bits::limit -> the final `out_pos != end_v || used_bits`; gzip: `pos > nb * 8u`", len(text), trunc=True)
    bad("truncated_in_stored_data", Deflate().stored(rnd(62, 500), True).getvalue()[:300], "`from + len > in_off + in_len` (BGZF), `from + len > nb` (gzip)", 500,
        trunc=True)
    return out


def greedy_tail(lens, skip):
    return greedy_cl_ops(lens[skip:])


def unused_word(distance):
    """A block whose single-code set (the distance code, or the literal/length code) meets its other, unused code word."""
    d = Deflate()
    if distance:  # literals, a length, then the distance bit: 0 is the code, 1 is not
        ll = lens_of(258, {97: 1, 256: 2, 257: 2})
        d.dynamic([97, 97, 97, 97], False, lit_lens=ll, dist_lens=[1], eob=False)
        d.bits(0b11, 2)  # length symbol 257 (canonical code 11)
        d.bits(1, 1)     # the distance code's unused word
    else:
        ll = lens_of(257, {256: 1})
        d.dynamic([], False, lit_lens=ll, dist_lens=[0], eob=False)
        d.bits(1, 1)     # the end of the block is 0; 1 is no code
    d.bits(0, 16)
    return d.getvalue()


VALID_GROUPS = {
    "code_shapes": code_shape_cases(),
    "empty_blocks": empty_block_cases(),
    "code_length_header": header_cases(),
    "fused_literals": fused_literal_cases(),
    "copies": copy_cases(),
    "stored": stored_cases(),
}
STRADDLE = straddle_cases()
VALID = [c for g in VALID_GROUPS.values() for c in g] + STRADDLE
INVALID = invalid_cases()
_random = {}


def _random_specs():
    if "specs" not in _random:
        _random["specs"] = random_specs()
    return _random["specs"]


def RANDOM():
    """The 300 random members of the BGZF route, one per block specification (built on first use: a second of Python)."""
    if "bgzf" not in _random:
        _random["bgzf"] = [of(f"random_{i}", render(spec)) for i, spec in enumerate(_random_specs())]
    return _random["bgzf"]


def RANDOM_GZIP():
    """The same 300 specifications for the gzip route: three in a row make one member of a few blocks (100 members; only the
    last block of a member is final, and a match may reach into the text of the specifications in front of its own)."""
    if "gzip" not in _random:
        specs = _random_specs()
        _random["gzip"] = [of(f"random_{i}_{i + 2}", render(specs[i] + specs[i + 1] + specs[i + 2])) for i in range(0, len(specs), 3)]
    return _random["gzip"]

"""A deflate WRITER for tests (RFC 1951): not a compressor, it writes exactly the blocks it is told to write, so that a test
can hand the device decoders (gmx_ingest.hip: ing_inflate_member, gz_decode) what zlib's compressor never emits: distances up
to 32 768, 15-bit codes, single-code distance sets, repeats across the HLIT / HDIST boundary, empty blocks, ... and damaged
streams. The tables below are copied from RFC 1951 §3.2.5, not computed the way the decoder computes them. Plain Python and
numpy; tests/test_deflate_craft_host.py pins everything written here to zlib's inflater."""
import heapq
import struct
import zlib

# RFC 1951 §3.2.5: length symbols 257..285 (extra bits, base length)
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
# distance symbols 0..29 (extra bits, base distance)
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
# §3.2.7: the order in which the code-length code's lengths are sent
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# §3.2.6: the fixed codes
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 32


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length 3..258; 258 is symbol 285."""
    if not 3 <= length <= 258:
        raise ValueError(f"match length {length}")
    if length == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        if LENGTH_BASE[i] <= length:
            return 257 + i, LENGTH_EXTRA[i], length - LENGTH_BASE[i]
    raise AssertionError


def distance_symbol(dist):
    """(symbol, extra bits, extra value) of a match distance 1..32768."""
    if not 1 <= dist <= 32768:
        raise ValueError(f"match distance {dist}")
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= dist:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise AssertionError


class Match:
    """A back-reference. lsym / dsym force the symbol: (284, extra 31) for length 258, or a raw distance symbol 30 / 31 (then
    `dist` is None and no extra bits follow)."""
    __slots__ = ("length", "dist", "lsym", "dsym")

    def __init__(self, length, dist, lsym=None, dsym=None):
        self.length, self.dist, self.lsym, self.dsym = length, dist, lsym, dsym


class RawLL:
    """A literal/length symbol by number, with nothing behind it (286, 287: no such symbol in the format)."""
    __slots__ = ("sym",)

    def __init__(self, sym):
        self.sym = sym


def _norm(tok):
    return Match(tok[0], tok[1]) if isinstance(tok, tuple) else tok


def expand(tokens):
    """The text the tokens stand for; overlapping copies byte by byte (RFC 1951 §3.2.3). ValueError for a distance that
    reaches before the start (and for a token that stands for no text)."""
    out = bytearray()
    for tok in tokens:
        if isinstance(tok, int):
            out.append(tok)
            continue
        if isinstance(tok, (bytes, bytearray)):
            out += tok
            continue
        m = _norm(tok)
        if not isinstance(m, Match) or m.dist is None:
            raise ValueError("a raw symbol stands for no text")
        if m.dist > len(out):
            raise ValueError(f"distance {m.dist} at position {len(out)} reaches before the start")
        if m.dist >= m.length:
            at = len(out) - m.dist
            out += out[at:at + m.length]
        else:
            for _ in range(m.length):
                out.append(out[-m.dist])
    return bytes(out)


def kraft(lens):
    """Kraft sum of the code lengths in units of 2^-15 (2^15: complete)."""
    return sum((1 << 15) >> l for l in lens if l)


def canonical_codes(lens):
    """Per symbol (code bits as they go into the stream, i.e. reversed; length) of the canonical code, RFC 1951 §3.2.2."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(None)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append((int(format(c & ((1 << l) - 1), f"0{l}b")[::-1], 2), l))  # (masked: an over-subscribed set, on request, overflows)
    return out


def limited_lengths(freqs, limit):
    """Code lengths of a Huffman code for the frequencies (0: no code), no length above `limit`, complete whenever two or more
    symbols are used (one symbol: a single code of one bit). Huffman's algorithm, then the Kraft sum repaired."""
    used = [s for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    tick = len(freqs)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tick, a + b))
        tick += 1
    for s in used:
        lens[s] = min(lens[s], limit)
    full = 1 << limit
    k = sum(full >> lens[s] for s in used)
    by_freq = sorted(used, key=lambda s: (freqs[s], s))
    while k > full:  # over-subscribed by the clamp: lengthen the rarest symbol that still can be
        s = next(s for s in by_freq if lens[s] < limit)
        k -= full >> (lens[s] + 1)
        lens[s] += 1
    while k < full:  # shorten the most frequent symbol whose gain fits
        s = next(s for s in reversed(by_freq) if lens[s] > 1 and (full >> lens[s]) <= full - k)
        k += full >> lens[s]
        lens[s] -= 1
    return lens


def expand_cl_ops(ops):
    """The code lengths a sequence of code-length symbols stands for: 0..15, (16, rep), (17, rep), (18, rep)."""
    out = []
    for op in ops:
        if isinstance(op, int):
            out.append(op)
            continue
        sym, rep = op
        if sym == 16:
            if not out:
                raise ValueError("16 as the first code-length symbol")
            out += [out[-1]] * rep
        else:
            out += [0] * rep
    return out


def greedy_cl_ops(lens, force=None):
    """Run-length encoding of the code lengths (§3.2.7), greedy; force = (sym, rep): the first run that can hold such a repeat
    starts with exactly that one."""
    ops, i, n = [], 0, len(lens)
    while i < n:
        v = lens[i]
        run = 1
        while i + run < n and lens[i + run] == v:
            run += 1
        left = run
        if v == 0:
            if force and force[0] in (17, 18) and left >= force[1]:
                ops.append(force)
                left -= force[1]
                force = None
            while left >= 11:
                r = min(left, 138)
                ops.append((18, r))
                left -= r
            if left >= 3:
                ops.append((17, left))
                left = 0
            ops += [0] * left
        else:
            ops.append(v)
            left -= 1
            if force and force[0] == 16 and left >= force[1]:
                ops.append(force)
                left -= force[1]
                force = None
            while left >= 3:
                r = min(left, 6)
                ops.append((16, r))
                left -= r
            ops += [v] * left
        i += run
    if force:
        raise ValueError(f"no run holds the repeat {force}")
    return ops


class Deflate:
    """One deflate stream, block by block. `tokens` collects what was written, for expand(); `block_bits` the bit at which every
    block starts (and the end of the last one)."""

    def __init__(self):
        self._acc, self._n, self._out = 0, 0, bytearray()
        self.tokens = []
        self.block_bits = [0]

    # ---- the bit writer: LSB first; Huffman codes arrive already reversed (canonical_codes) ----
    def bits(self, value, n):
        self._acc |= value << self._n
        self._n += n
        if self._n >= 2048:
            nb = self._n >> 3
            self._out += (self._acc & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little")
            self._acc >>= 8 * nb
            self._n &= 7

    def bit_pos(self):
        return len(self._out) * 8 + self._n

    def align(self):
        if self._n & 7:
            self.bits(0, 8 - (self._n & 7))

    def raw(self, data):
        self.align()
        nb = self._n >> 3
        self._out += self._acc.to_bytes(nb, "little")
        self._acc, self._n = 0, 0
        self._out += data

    def getvalue(self):
        n = (self._n + 7) >> 3
        return bytes(self._out) + self._acc.to_bytes(n, "little")

    def _done(self, tokens):
        self.tokens += tokens
        self.block_bits.append(self.bit_pos())
        return self

    # ---- blocks ----
    def stored(self, data, final=False, nlen=None, length=None):
        """A stored block; nlen: a wrong complement, length: a LEN other than len(data) (both on request only)."""
        data = bytes(data)
        ln = len(data) if length is None else length
        if len(data) > 65535 or not 0 <= ln <= 65535:
            raise ValueError("a stored block holds at most 65 535 bytes")
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.raw(struct.pack("<HH", ln, (ln ^ 0xFFFF) if nlen is None else nlen) + data)
        return self._done(list(data))

    def _symbols(self, tokens, lit, dist, eob):
        for tok in tokens:
            if isinstance(tok, int):
                c = lit[tok]
                if c is None:
                    raise ValueError(f"literal {tok} has no code")
                self.bits(*c)
                continue
            m = _norm(tok)
            if isinstance(m, RawLL):
                c = lit[m.sym] if m.sym < len(lit) else None
                if c is None:
                    raise ValueError(f"symbol {m.sym} has no code")
                self.bits(*c)
                continue
            if m.lsym is None:
                ls, le, lv = length_symbol(m.length)
            else:
                ls, le = m.lsym, LENGTH_EXTRA[m.lsym - 257]
                lv = m.length - LENGTH_BASE[m.lsym - 257]
                if not 0 <= lv < (1 << le) and not (le == 0 and lv == 0):
                    raise ValueError(f"length {m.length} is not in symbol {m.lsym}'s range")
            c = lit[ls] if ls < len(lit) else None
            if c is None:
                raise ValueError(f"length symbol {ls} has no code")
            self.bits(*c)
            if le:
                self.bits(lv, le)
            if m.dsym is None:
                ds, de, dv = distance_symbol(m.dist)
            else:
                ds, de, dv = m.dsym, 0, 0
            c = dist[ds] if ds < len(dist) else None
            if c is None:
                raise ValueError(f"distance symbol {ds} has no code")
            self.bits(*c)
            if de:
                self.bits(dv, de)
        if eob:
            if lit[256] is None:
                raise ValueError("the end-of-block symbol has no code")
            self.bits(*lit[256])

    def fixed(self, tokens, final=False, eob=True):
        """A block with the fixed codes (§3.2.6); RawLL(286 / 287) and Match(..., dsym=30 / 31) write the symbols the format lacks."""
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self._symbols(tokens, canonical_codes(FIXED_LIT_LENS), canonical_codes(FIXED_DIST_LENS), eob)
        return self._done(list(tokens))

    @staticmethod
    def used_symbols(tokens):
        lit, dist = [0] * 286, [0] * 30
        lit[256] = 1
        for tok in tokens:
            if isinstance(tok, int):
                lit[tok] += 1
                continue
            m = _norm(tok)
            if isinstance(m, RawLL):
                if m.sym < 286:
                    lit[m.sym] += 1
                continue
            lit[m.lsym if m.lsym is not None else length_symbol(m.length)[0]] += 1
            ds = m.dsym if m.dsym is not None else distance_symbol(m.dist)[0]
            if ds < 30:
                dist[ds] += 1
        return lit, dist

    def dynamic(self, tokens, final=False, lit_lens=None, dist_lens=None, cl_lens=None, cl_ops=None, hclen=None, invalid=False, eob=True,
                hlit=None, hdist=None, force=None):
        """A block with its own codes (§3.2.7). lit_lens (257..286 entries) / dist_lens (1..30 entries): the code lengths by
        symbol, or None: a length-limited Huffman code of the tokens. cl_ops: the code-length symbols that transmit them
        (expand_cl_ops), else a greedy run-length encoding (force: greedy_cl_ops). cl_lens: the code-length code's 19 lengths by
        symbol, else a Huffman code of the ops limited to 7 bits. hclen: how many of them are sent (4..19), else as few as
        possible. hlit / hdist: the header's counts when they are not to be the lists' lengths. Everything is checked (Kraft sums,
        every symbol used has a code, the ops give the lengths) unless invalid=True."""
        tokens = list(tokens)
        fl, fd = self.used_symbols(tokens)
        if lit_lens is None:
            lit_lens = limited_lengths(fl, 15)
            while len(lit_lens) > 257 and lit_lens[-1] == 0:
                lit_lens.pop()
        if dist_lens is None:
            dist_lens = limited_lengths(fd, 15)
            while len(dist_lens) > 1 and dist_lens[-1] == 0:
                dist_lens.pop()
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        n_lit = len(lit_lens) if hlit is None else hlit
        n_dist = len(dist_lens) if hdist is None else hdist
        if cl_ops is None:
            cl_ops = greedy_cl_ops(lit_lens + dist_lens, force)
        cl_ops = list(cl_ops)
        if cl_lens is None:
            f = [0] * 19
            for op in cl_ops:
                f[op if isinstance(op, int) else op[0]] += 1
            cl_lens = limited_lengths(f, 7)
            if sum(1 for l in cl_lens if l) == 1:  # (a single code-length code: give it a partner, complete sets only)
                cl_lens[0 if cl_lens[0] == 0 else 8] = 1
        cl_lens = list(cl_lens)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        if not invalid:
            def complete(lens, what, one_ok, none_ok=False):
                k, n = kraft(lens), sum(1 for l in lens if l)
                if not (k == 1 << 15 or (one_ok and n == 1 and k == 1 << 14) or (none_ok and n == 0)):
                    raise ValueError(f"{what}: Kraft sum {k} / 32768 with {n} codes")
            if not (257 <= n_lit <= 286 and 1 <= n_dist <= 30 and 4 <= hclen <= 19):
                raise ValueError("HLIT / HDIST / HCLEN out of range")
            if n_lit != len(lit_lens) or n_dist != len(dist_lens):
                raise ValueError("the header's counts are not the lists' lengths")
            if max(lit_lens + dist_lens) > 15 or max(cl_lens) > 7:
                raise ValueError("a code length beyond 15 (7 in the code-length code)")
            complete(lit_lens, "literal/length code", True)
            complete(dist_lens, "distance code", True, True)
            complete(cl_lens, "code-length code", False)
            if any(cl_lens[s] for s in CL_ORDER[hclen:]):
                raise ValueError("HCLEN cuts off a code-length code that is used")
            if any(not isinstance(op, int) and not {16: 3, 17: 3, 18: 11}[op[0]] <= op[1] <= {16: 6, 17: 10, 18: 138}[op[0]] for op in cl_ops):
                raise ValueError("a repeat count out of its symbol's range")
            if expand_cl_ops(cl_ops) != lit_lens + dist_lens:
                raise ValueError("the code-length symbols do not give the code lengths")
            if any(f and (s >= len(lit_lens) or not lit_lens[s]) for s, f in enumerate(fl)):
                raise ValueError("a literal/length symbol that is used has no code")
            if any(f and (s >= len(dist_lens) or not dist_lens[s]) for s, f in enumerate(fd)):
                raise ValueError("a distance symbol that is used has no code")
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(n_lit - 257, 5)
        self.bits(n_dist - 1, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lens[s], 3)
        cl = canonical_codes(cl_lens)
        for op in cl_ops:
            sym = op if isinstance(op, int) else op[0]
            if cl[sym] is None:
                raise ValueError(f"code-length symbol {sym} has no code")
            self.bits(*cl[sym])
            if sym == 16:
                self.bits(op[1] - 3, 2)
            elif sym == 17:
                self.bits(op[1] - 3, 3)
            elif sym == 18:
                self.bits(op[1] - 11, 7)
        lit = canonical_codes([min(l, 15) for l in lit_lens]) + [None] * (288 - len(lit_lens))
        dist = canonical_codes([min(l, 15) for l in dist_lens]) + [None] * (32 - len(dist_lens))
        self._symbols(tokens, lit, dist, eob)
        return self._done(tokens)

    def text(self):
        return expand(self.tokens)


# ---- wrappers ----
GZ_HDR = b"\x1f\x8b\x08\x00\0\0\0\0\0\xff"


def gzip_member(deflate_bytes, text, header=GZ_HDR, crc=None, isize=None):
    """RFC 1952: header, deflate data, CRC-32 and ISIZE of the text (or the wrong ones asked for)."""
    crc = zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc
    isize = len(text) & 0xFFFFFFFF if isize is None else isize
    return header + deflate_bytes + struct.pack("<II", crc, isize)


def padded_header(n):
    """A gzip header of n >= 11 bytes: FCOMMENT, with a comment that fills it."""
    return b"\x1f\x8b\x08\x10\0\0\0\0\0\xff" + b"c" * (n - 11) + b"\0"


def bgzf_member(deflate_bytes, text, crc=None, isize=None):
    """A BGZF member (SAM spec §4.1), the header layout of tests/test_ingest.py::bgzf."""
    crc = zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc
    isize = len(text) if isize is None else isize
    bsize = 12 + 6 + len(deflate_bytes) + 8
    if bsize > 65536:
        raise ValueError("a BGZF member holds at most 64 KB")
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1) + deflate_bytes +
            struct.pack("<II", crc, isize))


def bgzf_file(members):
    """Members (bytes of bgzf_member) in a row -> (the file, its members list (offset, size, isize, crc) in the form
    gramtools_amd.bgzf_members returns; here empty members are listed too)."""
    data, lst = bytearray(), []
    for m in members:
        crc, isize = struct.unpack("<II", m[-8:])
        lst.append((len(data) + 18, len(m) - 26, isize, crc))
        data += m
    return bytes(data), lst

// gmx_ingest_gzip.h — part of gmx_ingest.hip: plain gzip decoded in pieces.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------------------------------
// plain gzip (one deflate stream per member, members concatenated): the chunk's compressed bytes cut into PIECES decoded side
// by side, with the rules of gmx_pargz.h:
//   gmx_gz_decode_kernel   one wavefront per piece. The first piece of a file starts behind the gzip header, the first of a later
//                          chunk where the chunk before ended (on the device); any other piece searches a block start from its
//                          nominal bit: 64 bit positions at a time through the 17-bit screen, then a trial decode of the whole
//                          block (complete codes, text only, >= 1 KB, a plausible header behind it). Output: 16-bit symbols, a
//                          byte or "byte j of the 32 KB in front of the piece" (256 + j); back-references copy them along. The
//                          piece stops at the first block end at or beyond the next piece's nominal start; member ends (trailer,
//                          next header) are recorded on the way.
//   gmx_gz_link_kernel     one wavefront walks the pieces in order: a piece counts when it starts exactly where the one before
//                          ended; one that does not is decoded again from that end (the repair: all on the device). Text offsets.
//   gmx_gz_window_kernel   one block: the last 32 KB in front of every piece, in order (LDS, double-buffered)
//   gmx_gz_resolve_kernel  symbols -> bytes at the piece's text offset, where the record scan expects them
//   gmx_gz_crc_kernel      one wavefront per piece: CRC-32 of its text between member ends (and x^(8 n) to combine them)
//   gmx_gz_check_kernel    the parts combined in order and checked against every member's trailer (CRC-32 and ISIZE)
// ------------------------------------------------------------------------------------------------------------------
#define GZ_WIN 32768u    // deflate's window
#define GZ_ENDS 16u      // member ends one piece can record
#define GZ_RING 1024u    // 16-bit symbols in the LDS window (the 2 KB of WaveLds::ring)
#define GZ_RING_MASK (GZ_RING - 1u)
#define GZ_FLUSH 256u    // symbols per store of the window to memory (8 bytes per lane)
#define GZ_NEAR_MAX (GZ_RING - 320u)  // distances up to this are served from the LDS window
// what a piece's decode met (GzPiece::flags)
#define GZP_FOUND 1u     // decoding started (a searched start passed the block test)
#define GZP_EOS 2u       // the stream's end: the last member's trailer, then nothing or zeros
#define GZP_CAPPED 4u    // the piece's output passed its bound
#define GZP_OVERRUN 8u   // bytes needed beyond the chunk's (look-ahead included)
#define GZP_ENDS 16u     // more member ends than GZ_ENDS
#define GZP_BAD 32u      // not deflate / gzip here

struct GzPiece {
  uint32_t start, end;  // bits within the chunk's bytes: where decoding started, where it stopped
  uint32_t n_sym, flags, n_ends, text_off;
  uint32_t need, tail;  // bytes of the open member its matches need in front of the piece; symbols behind its last member end (all, when none)
  uint32_t end_at[GZ_ENDS], end_crc[GZ_ENDS], end_isize[GZ_ENDS];  // member ends: symbol index, the trailer's CRC-32 and ISIZE
  uint32_t seg_crc[GZ_ENDS + 1], seg_pow[GZ_ENDS + 1];             // the text between them: CRC register from 0, x^(8 length)
};
struct GzState {  // one per ingest: where the stream stands between chunks
  uint32_t bit;              // in the next chunk's bytes
  uint32_t eos;              // the stream has ended: what follows (from `bit` on) must be zeros
  uint32_t run_crc, run_len;  // the open member's CRC register and length so far
  uint32_t text_len;         // text of the chunk (the carry kernel's members_text)
  uint32_t flags;            // GMX_INGEST_* of the chunk
  uint32_t n_pieces;         // pieces in the chunk's chain
  uint32_t repairs;          // pieces decoded again from their predecessor's end, since the ingest was created
  uint32_t open;             // text of the open member at the chunk's end, saturated at GZ_WIN (run_len wraps with ISIZE: not that)
};
struct GzArgs {
  const uint32_t *comp;
  uint32_t n_bytes, n_own, final_chunk, fresh;
  uint32_t piece_bits, n_pieces, cap;  // nominal piece length; pieces; symbols a piece may write
  uint16_t *sym;
  GzPiece *pieces;
  GzState *st;
  uint32_t debug;               // GMX_GZ_DEBUG=1: the link kernel prints every piece
  uint32_t late_mod, drop_mod;  // test hook (GMX_GZ_TEST_FIND): pieces i % late_mod == 0 take the block start behind the true one,
                                // pieces i % drop_mod == drop_mod - 1 find none
};
typedef __attribute__((address_space(1))) uint16_t ing_g16;
typedef uint32_t ing_v2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) ing_v2 ing_g64;

__device__ __forceinline__ uint32_t gz_byte(const GzArgs &a, uint32_t at) { return at < a.n_bytes ? (uint32_t)reinterpret_cast<const uint8_t *>(a.comp)[at] : 0u; }
__device__ __forceinline__ uint32_t gz_le32(const GzArgs &a, uint32_t at) {
  return gz_byte(a, at) | gz_byte(a, at + 1u) << 8 | gz_byte(a, at + 2u) << 16 | gz_byte(a, at + 3u) << 24;
}
__device__ __forceinline__ uint32_t gz_stop_bit(const GzArgs &a, uint32_t i) {
  if (i + 1u < a.n_pieces) return (i + 1u) * a.piece_bits;
  return a.final_chunk ? 0xFFFFFFFFu : a.n_own * 8u;
}
// a gzip member header at byte `at` of b[0, n) (RFC 1952 §2.3): the byte behind it, or 0 with *why = GZP_BAD / GZP_OVERRUN
// (arguments by value: a reference to the kernel's GzArgs would put a copy of them in private memory, read per lane)
__device__ __attribute__((noinline)) uint32_t gz_header(const uint8_t *b, uint32_t n, uint32_t fin, uint32_t at, uint32_t *why) {
  auto byte = [&](uint32_t i) { return i < n ? (uint32_t)b[i] : 0u; };
  if (at + 10u > n) {
    *why = fin ? GZP_BAD : GZP_OVERRUN;
    return 0;
  }
  const uint32_t flg = byte(at + 3u);
  if (byte(at) != 0x1fu || byte(at + 1u) != 0x8bu || byte(at + 2u) != 8u || (flg & 0xE0u)) {
    *why = GZP_BAD;
    return 0;
  }
  uint32_t p = at + 10u;
  if (flg & 4u) p += 2u + (byte(p) | byte(p + 1u) << 8);  // FEXTRA
  if (flg & 8u) {                                        // FNAME
    while (p < n && byte(p)) ++p;
    ++p;
  }
  if (flg & 16u) {  // FCOMMENT
    while (p < n && byte(p)) ++p;
    ++p;
  }
  if (flg & 2u) p += 2u;  // FHCRC
  if (p > n) {
    *why = fin ? GZP_BAD : GZP_OVERRUN;
    return 0;
  }
  return p;
}
// bytes [at, n) of b all zero (the padding some writers leave behind the last member)
__device__ __attribute__((noinline)) bool gz_zeros(const uint8_t *b, uint32_t n, uint32_t at) {
  bool nz = false;
  for (uint32_t i = at + (threadIdx.x & 63u); i < n; i += 64u) nz = nz || b[i] != 0;
  return __ballot(nz) == 0;
}
__device__ __forceinline__ uint16_t gz_load_coherent(const ing_g16 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct GzDone {  // what gz_decode leaves (also in a.pieces[pi]; the link kernel goes on with these, not with its own stores)
  uint32_t flags, end, n_sym;
  uint32_t need, tail, n_ends;  // (GzPiece)
};
// Piece `pi` from bit `start` until a block ends at or beyond `stop` (or the stream ends). header_first: a member header stands at
// `start` (the file's first). trial: the first block must pass the block finder's tests (else the result is 0 and nothing is
// recorded). Results (lane 0's vector stores) into a.pieces[pi].
__device__ __forceinline__ GzDone gz_decode(WaveLds &L, const GzArgs &a, uint32_t pi, uint32_t start, bool header_first, bool trial, bool late) {
  const uint32_t lane = threadIdx.x & 63u;
  // (the values the scalar decoder works with are made wave-uniform first, as everything else in it)
  pi = uni(pi);
  start = uni(start);
  header_first = uni(header_first ? 1u : 0u) != 0;
  trial = uni(trial ? 1u : 0u) != 0;
  late = uni(late ? 1u : 0u) != 0;
  uint16_t *const ring = reinterpret_cast<uint16_t *>(L.ring);
  uint16_t *const dummy = reinterpret_cast<uint16_t *>(L.lens);  // (lens[] is dead in the symbol loop and the copies)
  ing_g16 *const out = (ing_g16 *)(a.sym + (size_t)pi * a.cap);
  GzPiece *const pc = a.pieces + pi;
  const uint32_t cap = uni(a.cap), stop = uni(gz_stop_bit(a, pi)), nb = uni(a.n_bytes), fin = uni(a.final_chunk);
  uint32_t out_pos = 0, flushed = 0, n_ends = 0, flags = GZP_FOUND, pos = start;
  int mstart = -(int)GZ_WIN;  // references may not reach below this (a member's first symbol: an empty window)
  int need = 0;               // how far the matches reach in front of the piece: the link kernel knows how much of the member lies there
  uint32_t last_end = 0;      // out_pos at the piece's last member end
  auto ring_reset = [&]() {  // the slots of positions [-1024, 0): placeholders for the window in front of the piece
    for (uint32_t k = lane; k < GZ_RING; k += 64u) ring[k] = (uint16_t)(256u + GZ_WIN - GZ_RING + k);
  };
  ring_reset();
  auto flush_to = [&](uint32_t upto) {  // [flushed, upto), upto a multiple of GZ_FLUSH
    for (uint32_t blk = flushed; blk < upto; blk += GZ_FLUSH)
      *(ing_g64 *)(out + blk + 4u * lane) = *reinterpret_cast<const ing_v2 *>(&ring[(blk + 4u * lane) & GZ_RING_MASK]);
    flushed = upto;
  };
  auto flush_rest = [&]() {  // [flushed, out_pos) symbol by symbol (`flushed` stays: the next flush_to stores them again, unchanged)
    for (uint32_t k = flushed + lane; k < out_pos; k += 64u) out[k] = ring[k & GZ_RING_MASK];
  };
  auto copy_match = [&](uint32_t len, uint32_t dist) {
    uint32_t i0 = 0;
    if (dist > GZ_NEAR_MAX) {  // from the symbols already stored (every position read lies below `flushed`), or the window's placeholders
      do {
        const uint32_t i = i0 + lane;
        const int src = (int)(out_pos - dist + i);
        const uint16_t v = src < 0 ? (uint16_t)(256 + (int)GZ_WIN + src) : gz_load_coherent(out + min((uint32_t)src, out_pos));
        *(i < len ? &ring[(out_pos + i) & GZ_RING_MASK] : &dummy[lane]) = v;
        i0 += 64u;
      } while (i0 < len);
    } else if (dist >= len) {
      do {
        const uint32_t i = i0 + lane;
        const uint16_t v = ring[(out_pos - dist + i) & GZ_RING_MASK];
        *(i < len ? &ring[(out_pos + i) & GZ_RING_MASK] : &dummy[lane]) = v;
        i0 += 64u;
      } while (i0 < len);
    } else {
      do {
        const uint32_t i = i0 + lane;
        const uint16_t v = ring[(out_pos - dist + i % dist) & GZ_RING_MASK];
        *(i < len ? &ring[(out_pos + i) & GZ_RING_MASK] : &dummy[lane]) = v;
        i0 += 64u;
      } while (i0 < len);
    }
    out_pos += len;
    if ((out_pos & ~(GZ_FLUSH - 1u)) > flushed) flush_to(out_pos & ~(GZ_FLUSH - 1u));
  };
  Bits bs;
  bs.limit = (nb + 3u) / 4u;  // (the words behind the chunk's bytes read as zero)
  if (header_first) {
    uint32_t why = 0;
    const uint32_t p = uni(gz_header(reinterpret_cast<const uint8_t *>(a.comp), nb, fin, start >> 3, &why));
    if (!p) {
      flags |= uni(why);
      goto done;
    }
    pos = p * 8u;
    mstart = 0;
  }
  bs.start(a.comp, pos >> 3);
  bs.drop(pos & 7u);
  for (bool first = true;; first = false) {
    bs.refill();
    const uint32_t last = bs.take(1), btype = bs.take(2);
    uint32_t bad = 0;
    if (btype == 0) {  // stored
      bs.drop(bs.cnt & 7u);
      bs.refill();
      const uint32_t len = bs.take(16), nlen = bs.take(16);
      const uint32_t from = bs.byte_pos();
      if ((len ^ nlen) != 0xFFFFu) {
        bad = GZP_BAD;
      } else if (from + len > nb) {
        bad = fin ? GZP_BAD : GZP_OVERRUN;
      } else if (out_pos + len > cap) {
        bad = GZP_CAPPED;
      } else {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(a.comp) + from;
        for (uint32_t i0 = 0; i0 < len; i0 += 64u) {
          const uint32_t n = min(64u, len - i0);
          *(lane < n ? &ring[(out_pos + lane) & GZ_RING_MASK] : &dummy[lane]) = src[i0 + min(lane, n - 1u)];
          out_pos += n;
          if ((out_pos & ~(GZ_FLUSH - 1u)) > flushed) flush_to(out_pos & ~(GZ_FLUSH - 1u));
        }
        bs.start(a.comp, from + len);
      }
    } else if (btype == 3u) {
      bad = GZP_BAD;
    } else if (ing_block_tables(L, bs, btype, trial && first)) {
      bad = GZP_BAD;
    } else {
      ing_fuse(L.lit, ING_LIT_ROOT);
      uint32_t stop_c = 0;  // 1 damaged, 2 the block's end, 3 the piece's bound
      do {
        bs.refill();
        uint32_t e = uni(L.lit[ing_vpeek<ING_LIT_ROOT>((uint32_t)bs.buf)]);
        if (__builtin_expect((int32_t)e < 0, 0)) {
          const uint64_t rr = ing_rare(0, e, bs.buf, L.lit_count, L.lit_sorted);
          const uint32_t r_lo = uni((uint32_t)rr);
          bs.drop(r_lo & 0xFFu);
          stop_c = r_lo >> 8;
          e = uni((uint32_t)(rr >> 32));
        }
        if ((e & ING_LENGTH) == 0) {
          const uint32_t n_lit = (e >> 6) & 3u;
          bs.drop(e & 15u);
          if (__builtin_expect(out_pos + n_lit > cap, 0)) {
            stop_c = 3u;
          } else {
            *(lane < n_lit ? &ring[(out_pos + lane) & GZ_RING_MASK] : &dummy[lane]) = (uint16_t)((e >> (8u + 8u * (lane & 3u))) & 0xFFu);
            out_pos += n_lit;
            if (__builtin_expect((out_pos & ~(GZ_FLUSH - 1u)) > flushed, 0)) flush_to(out_pos & ~(GZ_FLUSH - 1u));
          }
        } else {
          const uint32_t len = ((e >> 6) & 0x1FFu) + ing_sbfe((uint32_t)bs.buf, e);
          bs.drop(e >> 23);
          bs.refill();
          const uint64_t de = L.dist[ing_vpeek<ING_DIST_ROOT>((uint32_t)bs.buf)];
          const uint32_t d = uni((uint32_t)de);
          uint32_t dist;
          if (__builtin_expect((int32_t)d < 0, 0)) {
            const uint64_t rr = ing_rare(1, d, bs.buf, L.dist_count, L.dist_sorted);
            const uint32_t r_lo = uni((uint32_t)rr);
            bs.drop(r_lo & 0xFFu);
            stop_c = r_lo >> 8;
            dist = uni((uint32_t)(rr >> 32));
          } else {
            dist = uni((uint32_t)(de >> 32)) + ing_sbfe((uint32_t)bs.buf, d);
            bs.drop(d >> 23);
          }
          if (__builtin_expect((int)(out_pos - dist) < mstart, 0)) {
            stop_c = 1u;
          } else if (__builtin_expect(out_pos + len > cap, 0)) {
            stop_c = 3u;
          } else {
            need = max(need, (int)(dist - out_pos));
            copy_match(len, dist);
          }
        }
        asm volatile("" : "+s"(stop_c));
      } while (stop_c == 0);
      bad = stop_c == 1u ? GZP_BAD : stop_c == 3u ? GZP_CAPPED : 0u;
    }
    pos = bs.next_word() * 32u - bs.cnt;
    if (pos > nb * 8u) bad = fin ? GZP_BAD : GZP_OVERRUN;  // (zeros decoded from behind the bytes: whatever else went wrong came of that)
    if (trial && first) {  // the block finder's tests: a whole non-final block of >= 1 KB of text, a plausible header behind it
      bool ok = !bad && !last && out_pos >= 1024u;
      if (ok) {
        flush_rest();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        bool nt = false;
        for (uint32_t k = lane; k < out_pos; k += 64u) {
          const uint32_t c = gz_load_coherent(out + k);
          nt = nt || (c < 256u && !((c >= 0x20u && c < 0x7Fu) || c == '\n' || c == '\r' || c == '\t'));
        }
        ok = __ballot(nt) == 0;
      }
      if (ok) {
        Bits nx = bs;
        nx.refill();
        const uint32_t h = nx.take(3), type = h >> 1;
        if (type == 3u) {
          ok = false;
        } else if (type == 2u) {
          ok = nx.take(5) <= 29u && nx.take(5) <= 29u;
        } else if (type == 0u) {
          nx.drop(nx.cnt & 7u);
          nx.refill();
          const uint32_t len = nx.take(16), nlen = nx.take(16);
          ok = (len ^ nlen) == 0xFFFFu;
        }
      }
      if (!ok) return GzDone{0u, 0u, 0u, 0u, 0u, 0u};
      if (late) {  // test hook: a wrong (later) start, the link kernel has to repair it
        start = pos;
        out_pos = flushed = 0;
        need = 0;
        ring_reset();
      }
    }
    if (bad) {
      flags |= bad;
      break;
    }
    if (last) {  // the member's trailer (RFC 1952 §2.3), then another member or the stream's end
      bs.drop(bs.cnt & 7u);
      uint32_t at = (bs.next_word() * 32u - bs.cnt) / 8u;
      if (at + 8u > nb) {
        flags |= fin ? GZP_BAD : GZP_OVERRUN;
        break;
      }
      if (n_ends == GZ_ENDS) {
        flags |= GZP_ENDS;
        break;
      }
      const uint32_t crc = gz_le32(a, at), isize = gz_le32(a, at + 4u);
      if (lane == 0) {
        pc->end_at[n_ends] = out_pos;
        pc->end_crc[n_ends] = crc;
        pc->end_isize[n_ends] = isize;
      }
      ++n_ends;
      last_end = out_pos;
      at += 8u;
      pos = at * 8u;
      if (at + 3u <= nb && uni(gz_byte(a, at) | gz_byte(a, at + 1u) << 8 | gz_byte(a, at + 2u) << 16) == 0x088b1fu) {
        uint32_t why = 0;
        const uint32_t p = uni(gz_header(reinterpret_cast<const uint8_t *>(a.comp), nb, fin, at, &why));
        if (!p) {
          flags |= uni(why);
          break;
        }
        pos = p * 8u;
        mstart = (int)out_pos;
        bs.start(a.comp, p);
      } else if (uni(gz_zeros(reinterpret_cast<const uint8_t *>(a.comp), nb, at) ? 1u : 0u)) {  // nothing more, or zeros: the end
        flags |= GZP_EOS;
        break;
      } else {
        flags |= (!fin && at + 3u > nb) ? GZP_OVERRUN : GZP_BAD;
        break;
      }
    }
    if (pos >= stop) break;
  }
done:
  if ((out_pos & ~(GZ_FLUSH - 1u)) > flushed) flush_to(out_pos & ~(GZ_FLUSH - 1u));
  flush_rest();
  if (lane == 0) {
    pc->start = start;
    pc->end = pos;
    pc->n_sym = out_pos;
    pc->flags = flags;
    pc->n_ends = n_ends;
    pc->need = (uint32_t)need;
    pc->tail = out_pos - last_end;
  }
  return GzDone{uni(flags), uni(pos), uni(out_pos), uni((uint32_t)need), uni(out_pos - last_end), uni(n_ends)};
}

// one wavefront per piece: its start (known, or searched), then its symbols
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ING_WAVES, 8))) gmx_gz_decode_kernel(GzArgs a) {
  __shared__ WaveLds L;
  const uint32_t i = blockIdx.x, lane = threadIdx.x & 63u;
  if (i >= a.n_pieces || (!a.fresh && a.st->eos)) return;
  if (i == 0) {
    (void)gz_decode(L, a, 0, a.fresh ? 0u : a.st->bit, a.fresh != 0, false, false);
    return;
  }
  const bool late = uni(a.late_mod && i % a.late_mod == 0 ? 1u : 0u) != 0, drop = uni(a.drop_mod && i % a.drop_mod == a.drop_mod - 1u ? 1u : 0u) != 0;
  const uint32_t lo = uni(i * a.piece_bits), hi = uni(min((i + 1u) * a.piece_bits, a.n_own * 8u));
  const uint32_t n_words = uni((a.n_bytes + 3u) / 4u);
  for (uint32_t base = lo; base < hi && !drop; base += 64u) {
    // the 17-bit screen at 64 positions: BFINAL 0, BTYPE 10b, HLIT <= 29, HDIST <= 29; then, lane by lane, the code-length
    // code behind it must be complete (its HCLEN + 4 lengths of 3 bits: Kraft sum 1) — most chance positions fail here, before
    // a trial decode costs the wave a table build
    const uint32_t b = base + lane;
    auto bits64 = [&](uint32_t at) {  // 64 bits of the chunk from bit `at`
      const uint32_t wi = at >> 5, sh = at & 31u;
      const uint64_t lo = (uint64_t)(wi + 1u < n_words ? a.comp[wi + 1u] : 0u) << 32 | (wi < n_words ? a.comp[wi] : 0u);
      const uint64_t hi3 = wi + 2u < n_words ? a.comp[wi + 2u] : 0u;
      return sh ? (lo >> sh) | (hi3 << (64u - sh)) : lo;
    };
    const uint64_t w = bits64(b);
    bool pass = b < hi && (w & 7u) == 4u && ((w >> 3) & 31u) <= 29u && ((w >> 8) & 31u) <= 29u;
    if (pass) {
      const uint32_t hclen = (uint32_t)((w >> 13) & 15u) + 4u;
      const uint64_t cl = bits64(b + 17u);
      uint32_t kraft = 0;
      for (uint32_t k = 0; k < hclen; ++k) {
        const uint32_t l = (uint32_t)(cl >> (3u * k)) & 7u;
        kraft += l ? 128u >> l : 0u;
      }
      pass = kraft == 128u;
    }
    unsigned long long m = __ballot(pass);
    while (m) {
      const uint32_t j = (uint32_t)__builtin_ctzll(m);
      m &= m - 1ull;
      if (uni(gz_decode(L, a, i, base + j, false, true, late).flags)) return;
    }
  }
  if (lane == 0) {  // no start: the link kernel decodes this piece from where the one before ended
    a.pieces[i].start = 0xFFFFFFFFu;
    a.pieces[i].flags = 0;
    a.pieces[i].n_sym = 0;
    a.pieces[i].n_ends = 0;
  }
}

// One wavefront: the chain of pieces in stream order, repairs included; the chunk's text offsets and length.
__global__ void __launch_bounds__(64) gmx_gz_link_kernel(GzArgs a, uint64_t max_text) {
  __shared__ WaveLds L;
  const uint32_t lane = threadIdx.x & 63u;
  GzState *const st = a.st;
  if (a.fresh) {
    if (lane == 0) {
      st->eos = 0;
      st->run_crc = 0xFFFFFFFFu;
      st->run_len = 0;
      st->open = 0;
    }
    __syncthreads();
  }
  uint32_t flags = 0, n_chain = 0, repairs = 0;
  uint64_t text = 0;
  if (!a.fresh && uni(st->eos)) {  // the stream ended in a chunk before: zeros only
    if (!gz_zeros(reinterpret_cast<const uint8_t *>(a.comp), a.n_bytes, uni(st->bit) / 8u)) flags = GMX_INGEST_BAD_MEMBER;
    if (lane == 0) st->bit = uni(st->bit) > a.n_own * 8u ? uni(st->bit) - a.n_own * 8u : 0u;
  } else {
    uint32_t prev_end = 0, pf = 0;
    uint32_t open = a.fresh ? 0u : uni(st->open);  // text of the open member in front of the piece, saturated at 32 KB: all a match can reach
    for (uint32_t i = 0; i < a.n_pieces; ++i) {
      GzPiece *const pc = a.pieces + i;
      GzDone d{uni(pc->flags), uni(pc->end), uni(pc->n_sym), uni(pc->need), uni(pc->tail), uni(pc->n_ends)};  // (written by gmx_gz_decode_kernel)
      if (i > 0) {
        if (prev_end >= gz_stop_bit(a, i)) {  // a block of the piece before reaches over this piece's span: nothing left here
          d = GzDone{GZP_FOUND, prev_end, 0u, 0u, 0u, 0u};
          if (lane == 0) {
            pc->start = pc->end = prev_end;
            pc->n_sym = pc->n_ends = 0;
            pc->flags = GZP_FOUND;
          }
        } else if (!(d.flags & GZP_FOUND) || (d.flags & GZP_BAD) || uni(pc->start) != prev_end) {  // speculation that does not line up: decode it again
          d = gz_decode(L, a, i, prev_end, false, false, false);
          ++repairs;
          if (d.flags & GZP_BAD) flags |= GMX_INGEST_GZ_UNREPAIRED;
        }
      }
      pf = d.flags;
      if (a.debug && lane == 0) printf("[gz] piece %u: flags %u start %u end %u n_sym %u (stop %u, prev_end %u)\n", i, pf, pc->start, d.end, d.n_sym, gz_stop_bit(a, i), prev_end);
      if (pf & GZP_BAD) flags |= GMX_INGEST_BAD_MEMBER;
      if (pf & GZP_CAPPED) flags |= GMX_INGEST_GZ_PIECE_BOUND;
      if (pf & GZP_OVERRUN) flags |= a.final_chunk ? GMX_INGEST_BAD_MEMBER : GMX_INGEST_GZ_LOOKAHEAD;
      if (pf & GZP_ENDS) flags |= GMX_INGEST_GZ_MEMBER_ENDS;
      // a match may not reach in front of its member's first byte: within a piece mstart sees it, across pieces only the chain
      // knows how much of the member lies in front (the windows hold the text of earlier members, or zeros, there)
      if (!(pf & GZP_BAD) && d.need > open) flags |= GMX_INGEST_BAD_MEMBER;
      if (flags) break;
      open = min(d.n_ends ? d.tail : open + d.tail, GZ_WIN);
      if (lane == 0) pc->text_off = (uint32_t)text;
      text += d.n_sym;
      prev_end = d.end;
      n_chain = i + 1u;
      if (pf & GZP_EOS) break;
    }
    if (!flags) {
      if (pf & GZP_EOS) {
        if (!a.final_chunk && lane == 0) {  // (the trailer may lie in the look-ahead: the next chunk's zeros start behind it)
          st->eos = 1;
          st->bit = prev_end > a.n_own * 8u ? prev_end - a.n_own * 8u : 0u;
        }
      } else if (a.final_chunk) {
        flags = GMX_INGEST_BAD_MEMBER;  // the stream stops without its last member's trailer: truncated
      } else if (lane == 0) {
        st->bit = prev_end - a.n_own * 8u;
        st->open = open;
      }
      if (text > max_text) flags |= GMX_INGEST_GZ_TEXT_LIMIT;
    }
  }
  if (lane == 0) {
    st->flags = flags;
    st->text_len = flags ? 0u : (uint32_t)text;
    st->n_pieces = flags ? 0u : n_chain;
    st->repairs += repairs;
  }
}

// One block: the 32 KB in front of every piece (wins[i]), in stream order; the last 32 KB of the chunk's text for the next chunk.
__global__ void __launch_bounds__(1024) gmx_gz_window_kernel(GzArgs a, uint8_t *wins, uint8_t *window) {
  __shared__ uint8_t w[2][GZ_WIN];
  const uint32_t t = threadIdx.x;
  const GzState *st = a.st;
  const uint32_t n = st->n_pieces;
  if (st->flags || n == 0) return;
  for (uint32_t k = t * 16u; k < GZ_WIN; k += 16u * blockDim.x) *reinterpret_cast<uint4 *>(&w[0][k]) = a.fresh ? make_uint4(0, 0, 0, 0) : *reinterpret_cast<const uint4 *>(window + k);
  __syncthreads();
  uint32_t cur = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t *c = w[cur];
    uint8_t *nx = w[cur ^ 1u];
    for (uint32_t k = t * 16u; k < GZ_WIN; k += 16u * blockDim.x) *reinterpret_cast<uint4 *>(wins + (size_t)i * GZ_WIN + k) = *reinterpret_cast<const uint4 *>(c + k);
    const uint32_t len = a.pieces[i].n_sym;
    const uint16_t *s = a.sym + (size_t)i * a.cap;
    for (uint32_t k = t; k < GZ_WIN; k += blockDim.x) {
      const int q = (int)len - (int)GZ_WIN + (int)k;
      uint32_t v;
      if (q < 0) {
        v = c[GZ_WIN + q];
      } else {
        v = s[q];
        if (v >= 256u) v = c[v - 256u];
      }
      nx[k] = (uint8_t)v;
    }
    __syncthreads();
    cur ^= 1u;
  }
  for (uint32_t k = t * 16u; k < GZ_WIN; k += 16u * blockDim.x) *reinterpret_cast<uint4 *>(window + k) = *reinterpret_cast<const uint4 *>(&w[cur][k]);
}

// symbols -> bytes: blockIdx.x the piece, blockIdx.y its share
__global__ void __launch_bounds__(256) gmx_gz_resolve_kernel(GzArgs a, const uint8_t *wins, uint8_t *text) {
  const uint32_t i = blockIdx.x;
  const GzState *st = a.st;
  if (st->flags || i >= st->n_pieces) return;
  const uint32_t len = a.pieces[i].n_sym;
  uint8_t *const dst = text + a.pieces[i].text_off;
  const uint16_t *s = a.sym + (size_t)i * a.cap;
  const uint8_t *win = wins + (size_t)i * GZ_WIN;
  for (uint32_t q = blockIdx.y * blockDim.x + threadIdx.x; q < len; q += gridDim.y * blockDim.x) {
    const uint32_t v = s[q];
    dst[q] = v < 256u ? (uint8_t)v : win[v - 256u];
  }
}

// one wavefront per piece: the CRC register (from 0) of its text between member ends, and x^(8 length) to move a register past it
__global__ void __launch_bounds__(64) gmx_gz_crc_kernel(GzArgs a, const uint8_t *text) {
  __shared__ uint32_t crc_tab[1024];
  const uint32_t i = blockIdx.x, lane = threadIdx.x & 63u;
  const GzState *st = a.st;
  if (st->flags || i >= st->n_pieces) return;
  GzPiece *const pc = a.pieces + i;
  ing_crc_tables(crc_tab);
  const uint32_t n_ends = uni(pc->n_ends), n_sym = uni(pc->n_sym), off = uni(pc->text_off);
  for (uint32_t k = 0; k <= n_ends; ++k) {
    const uint32_t lo = k ? uni(pc->end_at[k - 1u]) : 0u, hi = k < n_ends ? uni(pc->end_at[k]) : n_sym;
    const uintptr_t p = (uintptr_t)(text + off + lo);
    const uint32_t first = (uint32_t)(p & 15u);
    const uint32_t c = ing_crc_wave(crc_tab, (const ing_g8 *)(p - first), first, first + (hi - lo), 0u);
    const uint32_t pw = ing_xpow8(hi - lo);
    if (lane == 0) {
      pc->seg_crc[k] = c;
      pc->seg_pow[k] = pw;
    }
  }
}

// one lane: the parts combined in stream order, every member's CRC-32 and ISIZE checked; the chunk's status for gmx_layout_kernel
__global__ void __launch_bounds__(64) gmx_gz_check_kernel(GzArgs a, IngestInflateStatus *inf) {
  if (threadIdx.x != 0) return;
  GzState *const st = a.st;
  uint32_t flags = st->flags;
  if (!flags) {
    uint32_t r = st->run_crc, len = st->run_len;
    for (uint32_t i = 0; i < st->n_pieces && !flags; ++i) {
      const GzPiece &pc = a.pieces[i];
      for (uint32_t k = 0; k <= pc.n_ends; ++k) {
        const uint32_t lo = k ? pc.end_at[k - 1u] : 0u, hi = k < pc.n_ends ? pc.end_at[k] : pc.n_sym;
        r = ing_mulmod(r, pc.seg_pow[k]) ^ pc.seg_crc[k];
        len += hi - lo;
        if (k < pc.n_ends) {
          if (~r != pc.end_crc[k] || len != pc.end_isize[k]) {
            flags |= GMX_INGEST_BAD_CRC;
            break;
          }
          r = 0xFFFFFFFFu;
          len = 0;
        }
      }
    }
    st->run_crc = r;
    st->run_len = len;
    if (flags) {
      st->flags = flags;
      st->text_len = 0;
    }
  }
  inf->flags = flags;
  inf->bad_member = flags ? 0u : 0xFFFFFFFFu;
}

}  // namespace

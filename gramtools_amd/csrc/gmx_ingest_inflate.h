// gmx_ingest_inflate.h — part of gmx_ingest.hip: the deflate decoder of BGZF members (tables, bit reader, CRC, gmx_inflate_kernel).
#pragma once

namespace {

#ifndef ING_LIT_ROOT
#define ING_LIT_ROOT 10
#endif
#ifndef ING_DIST_ROOT
#define ING_DIST_ROOT 7
#endif
#ifndef ING_RING
#define ING_RING 2048u
#endif
#ifndef ING_WAVES
#define ING_WAVES 5
#endif
#define ING_RING_MASK (ING_RING - 1u)
#define ING_NEAR_MAX (ING_RING - 320u)  // distances up to this are served from the LDS window

// table entry (32 bits): bits 0-3 the bits its code takes (0: no code here), bit 31 ING_RARE, and
//   literals     (literal/length table) bits 6-7 how many (ing_fuse: up to three literals whose codes fit the root bits together
//                take ONE look-up; 0: the entry that does nothing), bits 8-31 the bytes, first one lowest; bits 4-5 clear
//   length       (literal/length table) bit 5 (ING_LENGTH), bits 6-14 base value, bits 16-18 extra bits, bits 23-27 code + extra
//                bits: the entry itself is the operand of s_bfe_u32 that takes the extra bits out of the stream (offset = bits
//                0-4, width = bits 16-22), and one shift drops code and extra bits together
//   distance     (distance table) bit 4, bits 8-11 extra bits, bits 12-27 base value
//   code length  bits 8-12 the symbol
//   ING_RARE     bits 4-5 say which: ING_T_EOB, ING_T_LONG (a code longer than the table's bits), else no code
#define ING_T_LIT 0u
#define ING_T_BASE 1u
#define ING_T_EOB 2u
#define ING_T_LONG 3u
#define ING_TYPE(e) (((e) >> 4) & 3u)  // of an ING_RARE entry
#define ING_LENGTH 32u
#define ING_IS_LIT(e) (((e) & (ING_RARE | 48u)) == 0)
#define ING_RARE 0x80000000u  // set in every entry that is not a literal or a length / distance base: no code, end of block, longer code
                               // (a third fused literal is below 0x80, so that its byte does not reach the bit)

struct WaveLds {  // 8 KB: twenty wavefronts per CU
  uint32_t lit[1u << ING_LIT_ROOT];    // literal/length codes of up to ING_LIT_ROOT bits, by the next bits of the stream (4 KB); the CRC table afterwards
  uint64_t dist[1u << ING_DIST_ROOT];  // distance codes (1 KB, entries of two words); as 32-bit entries the code-length code while a dynamic block's lengths are read
  alignas(16) uint8_t ring[ING_RING];  // the last 2 KB of the member's text
  uint16_t lit_sorted[288];            // symbols by (code length, symbol): codes longer than the root are decoded bit by bit
  uint16_t dist_sorted[32];
  uint16_t lit_count[16], dist_count[16];
  union {
    uint8_t lens[320];                 // code lengths of the block being set up
    uint8_t dummy[64];                 // in the symbol loop (lens[] is dead then): where a lane with nothing to write writes, no lane-divergent branch
  };
};
static_assert(sizeof(WaveLds) <= 8192, "twenty wavefronts per CU");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// the low N bits of a wave-uniform word, computed on the vector unit (the table index of a look-up: the scalar unit is what
// bounds the decoder, the address has to be in a vector register anyway)
template <uint32_t N>
__device__ __forceinline__ uint32_t ing_vpeek(uint32_t v) {
  uint32_t r;
  asm("v_bfe_u32 %0, %1, 0, %2" : "=v"(r) : "s"(v), "n"(N));
  return r;
}
// bits [offset, offset + width) of v, offset = op bits 0-4, width = op bits 16-22 (the other bits of op are ignored): one scalar
// instruction where shift-and-mask by run-time amounts takes three
__device__ __forceinline__ uint32_t ing_sbfe(uint32_t v, uint32_t op) {
  uint32_t r;
  asm("s_bfe_u32 %0, %1, %2" : "=s"(r) : "s"(v), "s"(op) : "scc");
  return r;
}


// The bit reader. Everything but `cur` is wave-uniform. The compressed words are fetched 64 at a time, one per lane (a
// coalesced load; a single word per refill left the wave waiting a memory round trip every 32 bits) and taken, lane by
// lane, with v_readlane. No load stays in flight between refills: a prefetched next set made every iteration of the
// symbol loop wait for vector memory (its register copies), i.e. for every line of text flushed so far.
struct Bits {
  const uint32_t *w;
  uint32_t base;   // index of the word lane 0 holds in `cur`
  uint32_t rel;    // lane of `cur` that holds the next word to take (64: the next set is due)
  uint32_t cur;
  uint64_t buf;
  uint32_t cnt;
  uint32_t limit;  // words at and beyond this index are not the member's: never loaded, read as zero (set before start())
  __device__ __forceinline__ uint32_t fetch(uint32_t idx) const { return idx < limit ? w[idx] : 0u; }
  __device__ __forceinline__ void start(const uint32_t *words, uint32_t byte_off) {
    w = words;
    const uint32_t idx = byte_off >> 2, skip = (byte_off & 3u) * 8u;
    base = idx;
    cur = fetch(idx + threadIdx.x);
    buf = (uint64_t)(word_of(0) >> skip);
    cnt = 32u - skip;
    rel = 1u;
  }
  __device__ __forceinline__ uint32_t word_of(uint32_t lane_of) const {  // the word that lane holds
    return (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)lane_of);
  }
  __device__ __forceinline__ void refill() {  // afterwards at least 33 bits
    if (cnt <= 32u) {
      if (rel == 64u) {
        base += 64u;
        cur = fetch(base + threadIdx.x);  // (a truncated or damaged member decodes zeros from its end on: BAD_MEMBER below, nothing read beyond it)
        rel = 0;
      }
      buf |= (uint64_t)word_of(rel) << cnt;
      ++rel;
      cnt += 32u;
    }
  }
  __device__ __forceinline__ uint32_t next_word() const { return base + rel; }  // index of the next word to take
  __device__ __forceinline__ uint32_t peek(uint32_t n) const { return (uint32_t)buf & ((1u << n) - 1u); }
  __device__ __forceinline__ void drop(uint32_t n) {
    buf >>= n;
    cnt -= n;
  }
  __device__ __forceinline__ uint32_t take(uint32_t n) {
    const uint32_t v = peek(n);
    drop(n);
    return v;
  }
  __device__ __forceinline__ uint32_t byte_pos() const { return next_word() * 4u - cnt / 8u; }  // of the next unread bit's byte (cnt a multiple of 8)
};

// what a symbol of one of the three codes stands for, as a table entry of `len` bits
__device__ __forceinline__ uint32_t ing_entry(int kind, uint32_t s, uint32_t len) {
  if (kind == 0) {  // literal / length (RFC 1951 §3.2.5)
    if (s < 256u) return len | (1u << 6) | (s << 8);
    if (s == 256u) return len | (ING_T_EOB << 4) | ING_RARE;
    if (s > 285u) return ING_RARE;
    const uint32_t t = s - 257u;
    uint32_t base, extra;
    if (t < 8u) {
      base = 3u + t;
      extra = 0;
    } else if (t == 28u) {
      base = 258u;
      extra = 0;
    } else {
      extra = (t - 4u) >> 2;
      base = 3u + ((4u + (t & 3u)) << extra);
    }
    return len | ING_LENGTH | (base << 6) | (extra << 16) | ((len + extra) << 23);
  }
  return len | (ING_T_LIT << 4) | (s << 8);  // code-length code: the symbol itself
}

// distance symbol s as a table entry of `len` bits: low word = bits 0-3 len, bits 16-19 extra bits, bits 23-27 len + extra bits
// (the word is the s_bfe_u32 operand that takes the extra bits out of the stream); high word = base value. s > 29: ING_RARE
__device__ __forceinline__ uint64_t ing_dist_entry(uint32_t s, uint32_t len) {
  if (s > 29u) return ING_RARE;
  uint32_t base, extra;
  if (s < 4u) {
    base = 1u + s;
    extra = 0;
  } else {
    extra = (s - 2u) >> 1;
    base = 1u + ((2u + (s & 1u)) << extra);
  }
  return ((uint64_t)base << 32) | len | (extra << 16) | ((len + extra) << 23);
}

// Canonical Huffman code of lens[0, n) (RFC 1951 §3.2.2) -> look-up table of `root` bits + the sorted symbols and the
// counts per length for the bit-by-bit path. The wave works on 64 symbols at a time; a symbol's rank among those of its
// length comes from ballots. Returns false on an over-subscribed set of lengths.
__device__ __attribute__((noinline)) bool ing_build(const uint8_t *lens, uint32_t n, uint32_t *tab, uint32_t root, uint16_t *sorted, uint16_t *count, int kind) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long lt = (1ull << lane) - 1ull;
  uint64_t *const tab2 = reinterpret_cast<uint64_t *>(tab);  // kind 1: the distance table's entries have two words
  for (uint32_t i = lane; i < (1u << root); i += 64u) {
    if (kind == 1) tab2[i] = ING_RARE; else tab[i] = ING_RARE;
  }
  uint32_t cnt[16];
#pragma unroll
  for (int L = 0; L < 16; ++L) cnt[L] = 0;
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
#pragma unroll
    for (uint32_t L = 1; L <= 15u; ++L) cnt[L] += (uint32_t)__popcll(__ballot(l == L));
  }
  int left = 1;
#pragma unroll
  for (int L = 1; L <= 15; ++L) {
    left <<= 1;
    left -= (int)cnt[L];
    if (left < 0) return false;
  }
  uint32_t first[16], offs[16], run[16];
  {
    uint32_t code = 0, o = 0;
    first[0] = offs[0] = run[0] = 0;
#pragma unroll
    for (int L = 1; L <= 15; ++L) {
      code = (code + cnt[L - 1]) << 1;
      first[L] = code;
      offs[L] = run[L] = o;
      o += cnt[L];
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int L = 0; L < 16; ++L) count[L] = (uint16_t)cnt[L];
    count[0] = 0;
  }
  __syncthreads();  // (the zeroed table before the entries)
  for (uint32_t base = 0; base < n; base += 64u) {
    const uint32_t s = base + lane, l = s < n ? lens[s] : 0u;
    uint32_t my_at = 0, my_first = 0, my_offs = 0;
#pragma unroll
    for (uint32_t L = 1; L <= 15u; ++L) {
      const unsigned long long m = __ballot(l == L);
      if (l == L) {
        my_at = run[L] + (uint32_t)__popcll(m & lt);
        my_first = first[L];
        my_offs = offs[L];
      }
      run[L] += (uint32_t)__popcll(m);
    }
    if (l) {
      sorted[my_at] = (uint16_t)s;
      const uint32_t code = my_first + (my_at - my_offs);
      const uint32_t rev = __builtin_bitreverse32(code) >> (32u - l);
      if (l <= root) {
        if (kind == 1) {
          const uint64_t e = ing_dist_entry(s, l);
          for (uint32_t j = rev; j < (1u << root); j += 1u << l) tab2[j] = e;
        } else {
          const uint32_t e = ing_entry(kind, s, l);
          for (uint32_t j = rev; j < (1u << root); j += 1u << l) tab[j] = e;
        }
      } else if (kind == 1) {
        tab2[rev & ((1u << root) - 1u)] = 15u | (ING_T_LONG << 4) | ING_RARE;
      } else {
        tab[rev & ((1u << root) - 1u)] = 15u | (ING_T_LONG << 4) | ING_RARE;
      }
    }
  }
  __syncthreads();
  return true;
}

// Literal/length table: an entry whose literal leaves room in the root bits for the next code, when that is a literal too,
// becomes both (and a third): the bases of a FASTQ take two bits each, a run of one quality value one or two. The entry at j
// = the bits behind the first code does not depend on bits it does not cover, so T[i >> l1] IS the second look-up. In place,
// from the top down: an entry only looks at entries below itself, and a wave's LDS accesses keep their order.
__device__ __attribute__((noinline)) void ing_fuse(uint32_t *tab, uint32_t root) {
  const uint32_t lane = threadIdx.x & 63u;
  for (int c = (int)((1u << root) / 64u) - 1; c >= 0; --c) {
    const uint32_t i = (uint32_t)c * 64u + lane;
    uint32_t e = tab[i];
    uint32_t l = e & 15u;
    if (l != 0 && ING_IS_LIT(e) && l < root) {
      const uint32_t e2 = tab[i >> l], l2 = e2 & 15u;
      if (l2 != 0 && ING_IS_LIT(e2) && l + l2 <= root) {
        e = (l + l2) | (2u << 6) | (e & 0xFF00u) | ((e2 & 0xFF00u) << 8);
        l += l2;
        if (l < root) {
          const uint32_t e3 = tab[i >> l], l3 = e3 & 15u;
          if (l3 != 0 && ING_IS_LIT(e3) && l + l3 <= root && (e3 & 0x8000u) == 0) e = (l + l3) | (3u << 6) | (e & 0xFFFF00u) | ((e3 & 0xFF00u) << 16);
        }
      }
    }
    tab[i] = e;
  }
  __syncthreads();
}

// a code longer than the table's root: bit by bit against the canonical code's first code of every length. Out of line and
// by value (the symbol loop stays small): returns symbol | bits taken << 16, or ~0 when no code matches.
__device__ __attribute__((noinline)) uint32_t ing_decode_slow(uint64_t buf, const uint16_t *count, const uint16_t *sorted) {
  uint32_t code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= 15u; ++len) {
    code |= (uint32_t)(buf >> (len - 1u)) & 1u;
    const uint32_t c = uni(count[len]);
    if (code - first < c) return uni(sorted[index + (code - first)]) | (len << 16);
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return 0xFFFFFFFFu;
}

// What the symbol loop does with a table entry that has ING_RARE set (e: its low word), out of line and with ONE result.
// Low word: bits 0-7 bits to drop now, bits 8-9 the loop's `stop` (1 damaged, 2 the block's end). High word, literal/length
// table (kind 0): the entry the loop goes on with — the symbol's, as an entry of ONE bit (the code's other bits are the ones
// to drop now), or when stopping the entry that does nothing; distance table (kind 1): the distance itself, extra bits
// included (all of its bits are dropped now), 1 when stopping.
__device__ __attribute__((noinline)) uint64_t ing_rare(int kind, uint32_t e, uint64_t buf, const uint16_t *count, const uint16_t *sorted) {
  const uint64_t nop = (uint64_t)(kind == 0 ? 0u : 1u) << 32;
  const uint64_t bad = nop | (1u << 8);
  if ((e & 15u) == 0) return bad;                                             // no code here
  if (ING_TYPE(e) == ING_T_EOB) return nop | (2u << 8) | (e & 15u);             // the end of the block, from the table
  const uint32_t r = ing_decode_slow(buf, count, sorted);                     // a code longer than the table's bits
  if (r == 0xFFFFFFFFu) return bad;
  const uint32_t sym = r & 0xFFFFu, bits = r >> 16;
  if (kind == 1) {
    const uint64_t de = ing_dist_entry(sym, bits);
    if ((uint32_t)de & ING_RARE) return bad;
    const uint32_t extra = ((uint32_t)de >> 16) & 15u;
    const uint32_t dist = (uint32_t)(de >> 32) + ((uint32_t)(buf >> bits) & ((1u << extra) - 1u));
    return ((uint64_t)dist << 32) | (bits + extra);
  }
  const uint32_t e1 = ing_entry(0, sym, 1);
  if (e1 & ING_RARE) return (e1 & 15u) != 0 && ING_TYPE(e1) == ING_T_EOB ? nop | (2u << 8) | bits : bad;
  return ((uint64_t)e1 << 32) | (bits - 1u);
}

// Kraft sum of the code lengths lens[0, n) in units of 2^-15: 2^15 for a complete code (the block finder's test)
__device__ __attribute__((noinline)) uint32_t ing_kraft(const uint8_t *lens, uint32_t n) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t k = 0;
  for (uint32_t s = lane; s < n; s += 64u) k += lens[s] ? (1u << 15) >> lens[s] : 0u;
  for (int off = 32; off > 0; off >>= 1) k += __shfl_down(k, off);
  return uni(k);
}

// The code tables of a fixed (btype 1) or dynamic (btype 2) block whose three header bits the reader has taken: 0, or
// GMX_INGEST_BAD_MEMBER. `strict` (the gzip block finder): every code set complete as well.
__device__ __forceinline__ uint32_t ing_block_tables(WaveLds &L, Bits &bs, uint32_t btype, bool strict) {
  const uint32_t lane = threadIdx.x & 63u;
  if (btype == 1) {  // fixed codes (§3.2.6)
    for (uint32_t s0 = 0; s0 < 320u; s0 += 64u) {  // (lens[] has 320 entries; no lane-divergent branch inside the block loop, see the symbol loop)
      const uint32_t s = s0 + lane;
      L.lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
    }
    __syncthreads();
    bool ok = uni(ing_build(L.lens, 288, L.lit, ING_LIT_ROOT, L.lit_sorted, L.lit_count, 0)) != 0;
    L.lens[lane] = 5;  // (32 distance codes; the lanes above write lengths nobody reads)
    __syncthreads();
    ok = uni(ing_build(L.lens, 32, reinterpret_cast<uint32_t *>(L.dist), ING_DIST_ROOT, L.dist_sorted, L.dist_count, 1)) != 0 && ok;
    if (!ok) {
      return GMX_INGEST_BAD_MEMBER;
    }
  } else {  // dynamic codes (§3.2.7)
    // (while the lengths are read a lane with nothing to write writes into lit_sorted[]: the block before is done with it, this one
    // fills it when its lengths are complete; dummy[] shares its bytes with lens[])
    uint8_t *const hdr_dummy = reinterpret_cast<uint8_t *>(L.lit_sorted) + lane;
    const uint32_t hlit = bs.take(5) + 257u, hdist = bs.take(5) + 1u, hclen = bs.take(4) + 4u;
    if (hlit > 286u || hdist > 30u) {
      return GMX_INGEST_BAD_MEMBER;
    }
    *(lane < 19u ? &L.lens[lane] : hdr_dummy) = 0;
    __syncthreads();
    for (uint32_t i = 0; i < hclen; ++i) {
      bs.refill();
      const uint32_t v = bs.take(3);
      // order of the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
      const uint32_t sym = i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 8u - ((i - 3u) >> 1) : 8u + ((i - 4u) >> 1) + 0u;
      *(lane == 0 ? &L.lens[sym] : hdr_dummy) = (uint8_t)v;
    }
    __syncthreads();
    // (the code-length code's table borrows the distance table: root 7, every code at most 7 bits)
    uint32_t *const cl_tab = reinterpret_cast<uint32_t *>(L.dist);
    if (!uni(ing_build(L.lens, 19, cl_tab, 7, L.dist_sorted, L.dist_count, 2))) {
      return GMX_INGEST_BAD_MEMBER;
    }
    if (strict && uni(ing_kraft(L.lens, 19)) != (1u << 15)) return GMX_INGEST_BAD_MEMBER;
    const uint32_t total = hlit + hdist;
    uint32_t at = 0, prev = 0;
    while (at < total) {
      bs.refill();
      const uint32_t e = uni(cl_tab[bs.peek(7)]);
      if ((e & 15u) == 0) {
        return GMX_INGEST_BAD_MEMBER;
      }
      bs.drop(e & 15u);
      const uint32_t sym = e >> 8;
      uint32_t rep = 1, val = sym;
      if (sym == 16u) {
        if (at == 0) {
          return GMX_INGEST_BAD_MEMBER;
        }
        rep = 3u + bs.take(2);
        val = prev;
      } else if (sym == 17u) {
        rep = 3u + bs.take(3);
        val = 0;
      } else if (sym == 18u) {
        rep = 11u + bs.take(7);
        val = 0;
      }
      if (at + rep > total) {
        return GMX_INGEST_BAD_MEMBER;
      }
      for (uint32_t i0 = 0; i0 < rep; i0 += 64u) *(i0 + lane < rep ? &L.lens[at + i0 + lane] : hdr_dummy) = (uint8_t)val;  // (lens[0, 19) held the code-length code's lengths: its table is built)
      at += rep;
      prev = val;
    }
    for (uint32_t i0 = total; i0 < 320u; i0 += 64u) *(i0 + lane < 320u ? &L.lens[i0 + lane] : hdr_dummy) = 0;
    __syncthreads();
    if (uni(L.lens[256]) == 0) {  // no end-of-block code
      return GMX_INGEST_BAD_MEMBER;
    }
    if (strict) {  // complete literal/length code; a complete distance code, or a single distance code (RFC 1951 §3.2.7)
      const uint32_t kd = uni(ing_kraft(L.lens + hlit, hdist));
      if (uni(ing_kraft(L.lens, hlit)) != (1u << 15) || (kd != (1u << 15) && kd != (1u << 14))) return GMX_INGEST_BAD_MEMBER;
    }
    bool ok = uni(ing_build(L.lens, hlit, L.lit, ING_LIT_ROOT, L.lit_sorted, L.lit_count, 0)) != 0;
    ok = uni(ing_build(L.lens + hlit, hdist, reinterpret_cast<uint32_t *>(L.dist), ING_DIST_ROOT, L.dist_sorted, L.dist_count, 1)) != 0 && ok;
    if (!ok) {
      return GMX_INGEST_BAD_MEMBER;
    }
  }
  return 0;
}

// CRC-32 (IEEE, reflected) as polynomial arithmetic: a * b mod P, and x^n mod P (zlib's crc32_combine does the same)
#define ING_CRC_POLY 0xedb88320u
__device__ __forceinline__ uint32_t ing_mulmod(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & m) p ^= b;
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ ING_CRC_POLY : b >> 1;
  }
  return p;
}
__device__ __forceinline__ uint32_t ing_xpow8(uint32_t n_bytes) {  // x^(8 n)
  uint32_t base = 1u << 30;  // x^1
  base = ing_mulmod(base, base);
  base = ing_mulmod(base, base);
  base = ing_mulmod(base, base);  // x^8
  uint32_t r = 1u << 31;          // x^0
  while (n_bytes) {
    if (n_bytes & 1u) r = ing_mulmod(r, base);
    base = ing_mulmod(base, base);
    n_bytes >>= 1;
  }
  return r;
}

// The member's text is addressed as GLOBAL memory explicitly: through a generic pointer the stores were flat_store_byte,
// which count as LDS operations too — every table look-up behind a flushed line then waited for the line to reach memory.
typedef __attribute__((address_space(1))) uint8_t ing_g8;
typedef __attribute__((address_space(1))) uint32_t ing_g32;
typedef uint32_t ing_v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) ing_v4 ing_g128;
__device__ __forceinline__ uint8_t ing_load_coherent(const ing_g8 *p) {  // text this wave stored earlier: past the vector L1
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The four slicing-by-4 tables of CRC-32 (4 KB) into crc_tab (LDS), by the wave
__device__ __forceinline__ void ing_crc_tables(uint32_t *crc_tab) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t i = lane; i < 256u; i += 64u) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ ING_CRC_POLY : c >> 1;
    crc_tab[i] = c;
  }
  __syncthreads();
  for (uint32_t t = 1; t < 4u; ++t) {
    for (uint32_t i = lane; i < 256u; i += 64u) {
      const uint32_t v = crc_tab[(t - 1u) * 256u + i];
      crc_tab[t * 256u + i] = (v >> 8) ^ crc_tab[v & 0xFFu];
    }
    __syncthreads();
  }
}
// CRC register of bytes [first, total) of al (al 16-byte aligned): 64 slices side by side, four table look-ups per word, then the
// slices' registers combined pairwise; the register starts from `init` (0xFFFFFFFF: a member's CRC-32 is ~ the result; 0: the
// part's share, linear in its bytes, for ing_mulmod / ing_xpow8 to combine). Wave-uniform result.
__device__ __forceinline__ uint32_t ing_crc_wave(const uint32_t *crc_tab, const ing_g8 *al, uint32_t first, uint32_t total, uint32_t init) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t per = (((total + 63u) / 64u) + 3u) & ~3u;
  // (EVERY lane's slice starts at the member's first byte at the earliest — `first` bytes above the boundary: with only lane 0
  //  clamped, a member of a few hundred bytes that does not start on a 16-byte boundary had the bytes in front of it hashed
  //  by lanes 1.. and was reported as GMX_INGEST_BAD_CRC)
  uint32_t lo = min(total, max(first, lane * per));
  const uint32_t hi = max(lo, min(total, (lane + 1u) * per));
  uint32_t c = lane == 0 ? init : 0u;
  const uint32_t n = hi > lo ? hi - lo : 0u;
  auto byte_step = [&](uint32_t at) { c = crc_tab[(c ^ ing_load_coherent(al + at)) & 0xFFu] ^ (c >> 8); };
  while (lo < hi && (lo & 3u)) byte_step(lo++);
  const ing_g32 *words = (const ing_g32 *)al;
  for (; lo + 16u <= hi; lo += 16u) {  // four words in flight
    const uint32_t w0 = __hip_atomic_load(words + lo / 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                   w1 = __hip_atomic_load(words + lo / 4u + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                   w2 = __hip_atomic_load(words + lo / 4u + 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                   w3 = __hip_atomic_load(words + lo / 4u + 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t ws[4] = {w0, w1, w2, w3};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c ^= ws[q];
      c = crc_tab[768u + (c & 0xFFu)] ^ crc_tab[512u + ((c >> 8) & 0xFFu)] ^ crc_tab[256u + ((c >> 16) & 0xFFu)] ^ crc_tab[c >> 24];
    }
  }
  for (; lo + 4u <= hi; lo += 4u) {
    c ^= __hip_atomic_load(words + lo / 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c = crc_tab[768u + (c & 0xFFu)] ^ crc_tab[512u + ((c >> 8) & 0xFFu)] ^ crc_tab[256u + ((c >> 16) & 0xFFu)] ^ crc_tab[c >> 24];
  }
  while (lo < hi) byte_step(lo++);
  uint32_t nn = n;
  for (uint32_t dlt = 1; dlt < 64u; dlt <<= 1) {  // register of (left part || right part) = left * x^(8 |right|) + right
    const uint32_t c_r = __shfl_down(c, dlt), n_r = __shfl_down(nn, dlt);
    if ((lane & (2u * dlt - 1u)) == 0) {
      c = (n_r ? ing_mulmod(c, ing_xpow8(n_r)) : c) ^ c_r;
      nn += n_r;
    }
  }
  return uni(c);
}

// [lo, hi) within one KB of the window -> memory; the member's first and last pieces: a neighbour owns the rest of a 16-byte piece
__device__ __attribute__((noinline)) void ing_flush_partial(const uint8_t *ring, ing_g8 *al, uint32_t lo, uint32_t hi) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t cs = (lo & ~1023u) + 16u * lane, ce = cs + 16u;
  if (cs >= lo && ce <= hi) {
    *(ing_g128 *)(al + cs) = *reinterpret_cast<const ing_v4 *>(&ring[cs & ING_RING_MASK]);
  } else if (ce > lo && cs < hi) {
    for (uint32_t i = max(cs, lo); i < min(ce, hi); ++i) al[i] = ring[i & ING_RING_MASK];
  }
}

// One wavefront per member: its text goes to text[out_off, out_off + isize).
template <bool STATS>
__device__ __forceinline__ void ing_inflate_member(WaveLds &L, const uint32_t *__restrict__ comp, const IngestMember *__restrict__ members, uint32_t n_members,
                                                   uint8_t *text, IngestInflateStatus *st, int check_crc, unsigned long long *dbg, uint32_t exp_mode) {
  const uint32_t xm = STATS ? uni(exp_mode) : 0u;  // timing experiments (GMX_INGEST_EXP, with GMX_INGEST_STATS): the text is then wrong
  // dbg (GMX_INGEST_STATS=1): [0] look-ups of the literal/length table [1] literal bytes [2] matches [3] far matches [4] bit-by-bit
  // decodes [5] blocks [6..9] clocks: whole member, table building, match copies, CRC [10] members [11] match bytes
  unsigned long long n_look = 0, n_lit_total = 0, n_match = 0, n_far = 0, n_slow = 0, n_blocks = 0, t_build = 0, t_copy = 0, t_crc = 0, n_mbytes = 0;
  const long long t_begin = STATS ? clock64() : 0;
  const uint32_t mi = blockIdx.x;
  if (mi >= n_members) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t in_off = uni(members[mi].in_off), in_len = uni(members[mi].in_len), isize = uni(members[mi].isize);
  // Positions are counted from the 16-byte boundary at or below the member's first byte: byte p of that line-up lives at
  // al[p] and at ring[p & mask], so that a KB of the window goes to memory as one 16-byte store per lane (64-byte lines
  // stored byte by byte were 1 024 store instructions per member — and, loads and stores returning in order, every wait
  // for a load was a wait for the last of them).
  ing_g8 *const out0 = (ing_g8 *)(text + uni(members[mi].out_off));
  const uint32_t mis = (uint32_t)((uintptr_t)out0 & 15u);
  ing_g8 *const al = out0 - mis;
  const uint32_t end_v = isize + mis;
  Bits bs;
  bs.limit = (in_off + in_len + 3u) / 4u + 2u;  // (the member's words and the zeroed ones right behind them: ADVICE round 5 — the reader used to run on into the next member, or past the chunk's bytes)
  bs.start(comp, in_off);
  uint32_t out_pos = mis, flushed = mis;  // bytes decoded so far end here; bytes already stored from the window end here
  uint32_t err = 0;
  // The symbol loop below has only wave-uniform branches: a lane with nothing to do writes its byte to L.dummy instead of
  // sitting out a branch. (With lane-divergent branches and loops inside it the compiler restructured the whole loop around
  // flag registers: some 170 instruction slots per table look-up — and one wave issues an instruction every four clocks.)
  // (out of line: its branches are lane-divergent, and one divergent branch inside the symbol loop makes the compiler restructure
  // the whole loop around flag registers; with none the loop's wave-uniform branches stay plain scalar branches)
  auto flush_partial = [&](uint32_t lo, uint32_t hi) { ing_flush_partial(L.ring, al, lo, hi); };
  auto flush_to = [&](uint32_t upto) {  // [flushed, upto), upto a multiple of 1024
    if (xm & 4u) {
      flushed = upto;
      return;
    }
    uint32_t blk = flushed;
    if (blk & 1023u) {  // (once: the member's first KB starts at `mis`)
      flush_partial(blk, (blk & ~1023u) + 1024u);
      blk = (blk & ~1023u) + 1024u;
    }
    for (; blk < upto; blk += 1024u) *(ing_g128 *)(al + blk + 16u * lane) = *reinterpret_cast<const ing_v4 *>(&L.ring[(blk + 16u * lane) & ING_RING_MASK]);
    flushed = upto;
  };
  // bytes [out_pos, out_pos + len) = the len bytes starting dist back (RFC 1951 §3.2.3: may overlap what it writes); len >= 3.
  // Three loops that run at least once, so that the choice between them is two plain branches.
  auto copy_match = [&](uint32_t len, uint32_t dist) {
    if (xm & 1u) {
      out_pos += len;
      if ((out_pos & ~1023u) > flushed) flush_to(out_pos & ~1023u);
      return;
    }
    uint32_t i0 = 0;
    if (dist > ING_NEAR_MAX && !(xm & 2u)) {  // beyond the window: from the KBs already flushed (dist > 1 728: every byte read lies below `flushed`, for the idle lanes too)
      do {
        const uint32_t i = i0 + lane;
        const uint8_t v = ing_load_coherent(al + (out_pos - dist + i));
        uint8_t *dst = i < len ? &L.ring[(out_pos + i) & ING_RING_MASK] : &L.dummy[lane];
        *dst = v;
        i0 += 64u;
      } while (i0 < len);
    } else if (dist >= len) {  // from the window
      do {
        const uint32_t i = i0 + lane;
        const uint8_t v = L.ring[(out_pos - dist + i) & ING_RING_MASK];
        uint8_t *dst = i < len ? &L.ring[(out_pos + i) & ING_RING_MASK] : &L.dummy[lane];
        *dst = v;
        i0 += 64u;
      } while (i0 < len);
    } else {  // the copy overlaps what it writes: byte i repeats byte i mod dist
      do {
        const uint32_t i = i0 + lane;
        const uint8_t v = L.ring[(out_pos - dist + i % dist) & ING_RING_MASK];
        uint8_t *dst = i < len ? &L.ring[(out_pos + i) & ING_RING_MASK] : &L.dummy[lane];
        *dst = v;
        i0 += 64u;
      } while (i0 < len);
    }
    out_pos += len;
    if (__builtin_expect((out_pos & ~1023u) > flushed, 0)) flush_to(out_pos & ~1023u);
  };
  for (bool last = false; !last && !err;) {
    bs.refill();
    last = bs.take(1) != 0;
    const uint32_t btype = bs.take(2);
    if (STATS) ++n_blocks;
    const long long t_b0 = STATS ? clock64() : 0;
    if (btype == 0) {  // stored (RFC 1951 §3.2.4)
      bs.drop(bs.cnt & 7u);
      bs.refill();
      const uint32_t len = bs.take(16), nlen = bs.take(16);
      if ((len ^ nlen) != 0xFFFFu) {
        err = GMX_INGEST_BAD_MEMBER;
        break;
      }
      const uint32_t from = bs.byte_pos();
      if (from + len > in_off + in_len || out_pos + len > end_v) {
        err = GMX_INGEST_BAD_MEMBER;
        break;
      }
      const uint8_t *src = reinterpret_cast<const uint8_t *>(comp) + from;
      for (uint32_t i0 = 0; i0 < len; i0 += 64u) {
        const uint32_t n = min(64u, len - i0);
        *(lane < n ? &L.ring[(out_pos + lane) & ING_RING_MASK] : &L.dummy[lane]) = src[i0 + min(lane, n - 1u)];
        out_pos += n;
        if ((out_pos & ~1023u) > flushed) flush_to(out_pos & ~1023u);
      }
      bs.start(comp, from + len);
      continue;
    }
    if (btype == 3) {
      err = GMX_INGEST_BAD_MEMBER;
      break;
    }
    err = ing_block_tables(L, bs, btype, false);
    if (err) break;
    ing_fuse(L.lit, ING_LIT_ROOT);
    if (STATS) t_build += clock64() - t_b0;
    // ---- the block's symbols ----
    // The decoder is bound by the scalar instructions it issues (see below the function), so the loop is written the way the
    // compiler's control-flow passes leave alone: properly nested if / else, ONE way out at the bottom (`stop`, kept from the
    // optimizer so that it does not thread the rare cases to the code behind the loop), the rare cases out of line with one
    // result, nothing lane-divergent. As lambdas with early returns it carried its exits as a guard value and flag registers set
    // and tested on every path: 87 scalar instructions per match; this form takes 60-odd.
    {
      uint32_t stop = 0;  // 1: the member is damaged, 2: the block's end
      do {
        bs.refill();
        uint32_t e = uni(L.lit[ing_vpeek<ING_LIT_ROOT>((uint32_t)bs.buf)]);
        if (STATS) ++n_look;
        if (__builtin_expect((int32_t)e < 0, 0)) {  // ING_RARE: no code here, the end of the block, or a code longer than the table's bits
          if (STATS) ++n_slow;
          const uint64_t rr = ing_rare(0, e, bs.buf, L.lit_count, L.lit_sorted);
          const uint32_t r_lo = uni((uint32_t)rr);
          bs.drop(r_lo & 0xFFu);
          stop = r_lo >> 8;
          e = uni((uint32_t)(rr >> 32));  // (when stopping: the entry that does nothing)
        }
        if ((e & ING_LENGTH) == 0) {  // one to three literals (or none)
          const uint32_t n_lit = (e >> 6) & 3u;
          bs.drop(e & 15u);
          if (__builtin_expect(out_pos + n_lit > end_v, 0)) {
            stop = 1u;
          } else {
            uint8_t *dst = lane < n_lit ? &L.ring[(out_pos + lane) & ING_RING_MASK] : &L.dummy[lane];
            *dst = (uint8_t)(e >> (8u + 8u * (lane & 3u)));
            out_pos += n_lit;
            if (STATS) n_lit_total += n_lit;
            if (__builtin_expect((out_pos & ~1023u) > flushed, 0)) flush_to(out_pos & ~1023u);
          }
        } else {  // a length: its extra bits, then the distance code and its extra bits (RFC 1951 §3.2.5)
          const uint32_t len = ((e >> 6) & 0x1FFu) + ing_sbfe((uint32_t)bs.buf, e);
          bs.drop(e >> 23);
          bs.refill();
          const uint64_t de = L.dist[ing_vpeek<ING_DIST_ROOT>((uint32_t)bs.buf)];
          const uint32_t d = uni((uint32_t)de);
          uint32_t dist;
          if (__builtin_expect((int32_t)d < 0, 0)) {  // ING_RARE
            const uint64_t rr = ing_rare(1, d, bs.buf, L.dist_count, L.dist_sorted);
            const uint32_t r_lo = uni((uint32_t)rr);
            bs.drop(r_lo & 0xFFu);
            stop = r_lo >> 8;
            dist = uni((uint32_t)(rr >> 32));  // (when stopping: 1)
          } else {
            dist = uni((uint32_t)(de >> 32)) + ing_sbfe((uint32_t)bs.buf, d);
            bs.drop(d >> 23);
          }
          // (both in one test: every value is far below 2^31)
          if (__builtin_expect((int32_t)((out_pos - mis - dist) | (end_v - out_pos - len)) < 0, 0)) {
            stop = 1u;
          } else {
            if (STATS) {
              ++n_match;
              n_mbytes += len;
              if (dist > ING_NEAR_MAX) ++n_far;
            }
            const long long t_c0 = STATS ? clock64() : 0;
            copy_match(len, dist);
            if (STATS) t_copy += clock64() - t_c0;
          }
        }
        asm volatile("" : "+s"(stop));
      } while (stop == 0);
      if (stop == 1u) err = GMX_INGEST_BAD_MEMBER;
    }
  }
  if (!err) {
    if ((out_pos & ~1023u) > flushed) flush_to(out_pos & ~1023u);
    if (out_pos > flushed) {  // the member's last piece (and, for a member below one KB, its first)
      flush_partial(flushed, out_pos);
      flushed = out_pos;
    }
    // every byte of the member's deflate data used, and as much text as its trailer says
    const uint32_t used_bits = (bs.next_word() * 32u - bs.cnt) - in_off * 8u;
    if (out_pos != end_v || (used_bits + 7u) / 8u != in_len) err = GMX_INGEST_BAD_MEMBER;
  }
  const long long t_crc0 = STATS ? clock64() : 0;
  if (!err && check_crc && isize) {
    // CRC-32 of the member's text: 64 slices side by side, four table look-ups per word (the tables take the place of the
    // literal/length table), then the slices' registers combined pairwise. (One byte per step from memory — a memory round
    // trip each — was a third of the kernel's time.)
    static_assert(offsetof(WaveLds, ring) + ING_RING >= 4096u && offsetof(WaveLds, lit) == 0, "the four CRC tables take the place of the tables and the window");
    uint32_t *const crc_tab = reinterpret_cast<uint32_t *>(&L);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    ing_crc_tables(crc_tab);
    // slices of whole words, counted like everything else from the 16-byte boundary below the member's first byte
    const uint32_t c = ing_crc_wave(crc_tab, al, mis, end_v, 0xFFFFFFFFu);
    if (uni(~c) != uni(members[mi].crc)) err = GMX_INGEST_BAD_CRC;
  }
  if (STATS && dbg && lane == 0) {
    t_crc = clock64() - t_crc0;
    const unsigned long long v[12] = {n_look, n_lit_total, n_match, n_far, n_slow, n_blocks, (unsigned long long)(clock64() - t_begin), t_build, t_copy, t_crc, 1ull, n_mbytes};
    for (int i = 0; i < 12; ++i) atomicAdd(&dbg[i], v[i]);
  }
  if (err && lane == 0) {
    atomicOr(&st->flags, err);
    atomicMin(&st->bad_member, mi);
  }
}

// The decoder is ONE thread of control per wavefront, compiled scalar: it runs on the CU's single scalar unit, which all of
// the CU's wavefronts share. That unit is what bounds the kernel (profiles/round5/ingest_inflate_sq_counters.txt: 603 k scalar
// instructions per member, the scalar unit busy 68 % of the kernel's cycles; 4 or 7 waves per SIMD decode the same
// 30-34 GB/s of text). The same arithmetic compiled for the vector units — every lane redundantly — came out no faster: its
// branches cost as many scalar instructions (exec masks) as the scalar form's arithmetic. DESIGN.md §11: what comes next.
template <bool STATS>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ING_WAVES, 8)))
gmx_inflate_kernel(const uint32_t *__restrict__ comp, const IngestMember *__restrict__ members, uint32_t n_members, uint8_t *text, IngestInflateStatus *st,
                   int check_crc, unsigned long long *dbg, uint32_t exp_mode) {
  __shared__ WaveLds L;
  ing_inflate_member<STATS>(L, comp, members, n_members, text, st, check_crc, dbg, exp_mode);
}

}  // namespace

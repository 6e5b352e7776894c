// gmx_ingest.hip — reads files decoded ON the device (round 5; SURVEY.md §8f-3, VERDICT round 4 "missing" #4).
//
// The reference reads `.fastq.gz` through zlib / htslib on one host thread (libgramtools/include/sequence_read/seqread.hpp:94-180,
// src/genotype/quasimap/quasimap.cpp:65-76). The mapping kernels take 1 M reads in 0.4 ms; sixteen host cores inflate BGZF at
// 32-48 M reads/s. Here the compressed members go over PCIe as they lie in the file (a quarter of the text) and the GPU does
// the rest:
//
//   gmx_inflate_kernel     one wavefront per BGZF member (<= 64 KB of text, independent deflate streams, SAM spec §4.1): the
//                          Huffman tables of the member's blocks and a 4 KB window of its output live in LDS; the bit stream
//                          is decoded by the wave as ONE scalar thread of control (every value wave-uniform: the compiler
//                          keeps the bit buffer in SGPRs), match copies and line flushes use the 64 lanes; CRC-32 of the
//                          member's text by the same wave (64 slices, GF(2) combination), compared with the trailer's.
//   gmx_nl_count/_mark     newline positions of the chunk's text (tile counts -> scan -> positions)
//   gmx_records_kernel     four-line records: checks '@' / '+' / equal lengths, read lengths, one length for all or not
//   gmx_fq_pack_kernel     32 letters -> one pair of bit planes, in the layout gmx_pack_reads / the host parser produce
//                          (include/gmx.h), unencodable reads flagged in skip[] (encode_dna_bases, common/utils.cpp:73-92)
//   gmx_seq_lines1-3 / gmx_seq_records / gmx_seq_pack   FASTA and one-read-per-line text (gmx_ingest_set_format) in place of
//                          gmx_records / gmx_fq_pack: see "records whose sequence is not one line" below
//   gmx_bam_chain / _link / _scan1-2 / _records / _pack   BAM (binary records chained by their block_size) in place of the newline
//                          and record kernels: see "BAM" below
//
// A chunk's incomplete last record is carried into the next chunk on the device. Anything irregular (not four-line FASTQ, a
// damaged member, a CRC mismatch) is reported in gmx_ingest_result::status and decided by the caller (`gram` re-inflates the
// chunk with zlib and hands the text to gmx_ingest_submit_text, so a defect of this decoder cannot lose or invent reads).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gmx_internal.h"

#define ING_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      gmx_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
      return GMX_EHIP;                                                                     \
    }                                                                                      \
  } while (0)

namespace {

// ------------------------------------------------------------------------------------------------------------------
// device-side state of one chunk (one slot): written by the kernels, read by the next kernel and, at the end, by the host
// ------------------------------------------------------------------------------------------------------------------
struct IngestState {
  uint32_t text_start;     // first byte of the chunk's text in the slot's text buffer (carry of the chunk before included)
  uint32_t text_len;       // bytes from there
  uint32_t n_lines;        // complete lines (a last line without '\n' counts when the chunk is the file's last)
  uint32_t n_reads;
  uint32_t min_len, max_len;
  uint32_t flags;          // GMX_INGEST_* status bits
  uint32_t bad_member;     // first member that failed (index within the chunk)
  uint32_t consumed;       // bytes of text the records take
  uint32_t tail_len;       // text_len - consumed: carried into the next chunk
  uint32_t any_skip;
  uint32_t uniform_len;
  unsigned long long n_bases;
  unsigned long long n_pairs;
  unsigned long long sub_pairs[16];  // pair index of read i * 2^20 (offsets form): where a launch of <= 2^20 reads starts
  uint32_t final_chunk;
  uint32_t n_heads;        // FASTA / LINES: lines that start a record (gmx_seq_lines2_kernel)
};

struct IngestInflateStatus {  // written by gmx_inflate_kernel (a stream of its own), merged into the chunk's state by gmx_layout_kernel
  uint32_t flags, bad_member;
};

struct IngestMember {
  uint32_t in_off, in_len;   // deflate data within the chunk's compressed bytes
  uint32_t out_off, isize;   // its text within the chunk's text (from the first member's first byte)
  uint32_t crc, pad;
};

#define ING_CARRY_MAX (1u << 20)  // bytes of an incomplete last record that can be carried (a record longer than this: irregular)
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

// ------------------------------------------------------------------------------------------------------------------
// the chunk's text -> records -> bit planes
// ------------------------------------------------------------------------------------------------------------------
// starts a chunk: the incomplete last record of the chunk before (prev; null: a file's first chunk) in front of this one's text
__device__ __forceinline__ void ing_carry(const IngestState *prev, const uint8_t *prev_text, IngestState *cur, uint8_t *cur_text, uint32_t members_text,
                                          uint32_t final_chunk, uint32_t host_tail) {
  uint32_t tail = host_tail;  // (gmx_ingest_scan: the caller has put that many bytes in front of the chunk's text already)
  if (prev) {
    tail = prev->tail_len;
    if (tail > ING_CARRY_MAX) tail = 0;  // (reported below)
    const uint8_t *src = prev_text + prev->consumed;
    uint8_t *dst = cur_text + ING_CARRY_MAX - tail;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < tail; i += gridDim.x * blockDim.x) dst[i] = src[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    cur->text_start = ING_CARRY_MAX - tail;
    cur->text_len = tail + members_text;
    cur->n_lines = cur->n_reads = 0;
    cur->min_len = 0xFFFFFFFFu;
    cur->max_len = 0;
    cur->flags = (prev && prev->tail_len > ING_CARRY_MAX) ? GMX_INGEST_BAD_RECORD : 0u;
    cur->bad_member = 0xFFFFFFFFu;
    cur->consumed = ING_CARRY_MAX - tail;
    cur->tail_len = 0;
    cur->any_skip = 0;
    cur->uniform_len = 0;
    cur->n_bases = 0;
    cur->n_pairs = 0;
    for (int i = 0; i < 16; ++i) cur->sub_pairs[i] = 0;
    cur->final_chunk = final_chunk;
  }
}

__global__ void gmx_carry_kernel(const IngestState *prev, const uint8_t *prev_text, IngestState *cur, uint8_t *cur_text, uint32_t members_text,
                                 uint32_t final_chunk, uint32_t host_tail) {
  ing_carry(prev, prev_text, cur, cur_text, members_text, final_chunk, host_tail);
}
// the same for a plain gzip chunk: its text length is on the device (gmx_gz_link_kernel / gmx_gz_check_kernel)
__global__ void gmx_carry_gz_kernel(const IngestState *prev, const uint8_t *prev_text, IngestState *cur, uint8_t *cur_text, const uint32_t *members_text,
                                    uint32_t final_chunk) {
  ing_carry(prev, prev_text, cur, cur_text, *members_text, final_chunk, 0u);
}

#define ING_TILE 4096u  // bytes of text per 256-thread block of the newline kernels (16 per thread)
__device__ __forceinline__ uint32_t ing_nl_mask16(const uint8_t *text, uint32_t at, uint32_t lo, uint32_t hi) {  // bit j: text[at + j] == '\n', within [lo, hi)
  if (at + 16u <= lo || at >= hi) return 0u;
  const uint4 v = *reinterpret_cast<const uint4 *>(text + at);  // (at a multiple of 16; the buffer is padded)
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t t = w[q] ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);  // 0x80 in every zero byte, exactly
    m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
  }
  if (at < lo) m &= ~((1u << (lo - at)) - 1u);
  if (at + 16u > hi) m &= (1u << (hi - at)) - 1u;
  return m;
}
__global__ void __launch_bounds__(256) gmx_nl_count_kernel(const uint8_t *text, const IngestState *st, uint32_t *tile_count) {
  const uint32_t lo = st->text_start, hi = lo + st->text_len;
  const uint32_t at = blockIdx.x * ING_TILE + threadIdx.x * 16u;
  uint32_t c = (uint32_t)__popc(ing_nl_mask16(text, at, lo, hi));
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  __shared__ uint32_t part[4];
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// Exclusive scans in two levels, ONE WAVEFRONT per block and no LDS (round 5, second half). The chunk's result waits for these
// scans, and they run beside the inflate kernel of the next chunk, whose twenty wavefronts per CU hold all of the CU's LDS and five
// of a SIMD's eight wave slots: the single block of 1024 threads with 8 KB of LDS that did this until then found no CU to start on
// before that kernel's queue of workgroups ran dry (1.7-3.4 ms instead of 0.25). A wavefront without LDS fits beside them.
//   level 1 (a block per 1024 elements, 16 per lane): offsets within the block (out may alias in), the block's sum -> blk_tot
//   level 2 (one wavefront): blk_tot -> the blocks' offsets, in place; returns the total
// and whoever reads element i adds blk_tot[i >> 10].
#define ING_SCAN_BLOCK 1024u
template <class TIn, class TOut, class TTot>
__device__ __forceinline__ void ing_scan_level1(const TIn *in, TOut *out, uint32_t n, uint32_t blk, TTot *blk_tot) {
  const uint32_t lane = threadIdx.x & 63u, base = blk * ING_SCAN_BLOCK + lane * 16u;
  TTot v[16], sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16u; ++j) {
    v[j] = base + j < n ? (TTot)in[base + j] : (TTot)0;
    sum += v[j];
  }
  TTot incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const TTot up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  TTot run = incl - sum;
#pragma unroll
  for (uint32_t j = 0; j < 16u; ++j) {
    if (base + j < n) out[base + j] = (TOut)run;
    run += v[j];
  }
  if (lane == 63u) blk_tot[blk] = incl;
}
template <class TTot>
__device__ __forceinline__ TTot ing_scan_level2(TTot *blk_tot, uint32_t n_blk) {
  const uint32_t lane = threadIdx.x & 63u, per = (n_blk + 63u) / 64u;
  const uint32_t lo = min(n_blk, lane * per), hi = min(n_blk, lo + per);
  TTot sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += blk_tot[i];
  TTot incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const TTot up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  TTot run = incl - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    const TTot v = blk_tot[i];
    blk_tot[i] = run;
    run += v;
  }
  return __shfl(incl, 63);
}
__global__ void __launch_bounds__(64) gmx_tile_scan1_kernel(uint32_t *tile_count, uint32_t n_tiles, uint32_t *tile_blk) {
  ing_scan_level1<uint32_t, uint32_t, uint32_t>(tile_count, tile_count, n_tiles, blockIdx.x, tile_blk);
}
__global__ void __launch_bounds__(64) gmx_tile_scan2_kernel(uint32_t *tile_blk, uint32_t n_blk, IngestState *st, uint32_t cap_lines) {
  // (a tile holds at most 4096 newlines and a chunk's text at most 3 GB: the total fits 32 bits)
  const uint32_t total = ing_scan_level2<uint32_t>(tile_blk, n_blk);
  if (threadIdx.x == 0) {
    st->n_lines = total;
    if (total > cap_lines) atomicOr(&st->flags, GMX_INGEST_TOO_MANY_LINES);
  }
}
__global__ void __launch_bounds__(256) gmx_nl_mark_kernel(const uint8_t *text, const IngestState *st, const uint32_t *tile_base, const uint32_t *tile_blk,
                                                          uint32_t *line_end, uint32_t cap_lines) {
  if (st->flags & GMX_INGEST_TOO_MANY_LINES) return;
  const uint32_t lo = st->text_start, hi = lo + st->text_len;
  const uint32_t at = blockIdx.x * ING_TILE + threadIdx.x * 16u;
  uint32_t m = ing_nl_mask16(text, at, lo, hi);
  const uint32_t c = (uint32_t)__popc(m);
  uint32_t incl = c;  // inclusive scan over the block: within the wave by shuffles, across the four waves through LDS
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d);
    if ((int)(threadIdx.x & 63u) >= d) incl += up;
  }
  __shared__ uint32_t wsum[4];
  if ((threadIdx.x & 63u) == 63u) wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t before = tile_blk[blockIdx.x / ING_SCAN_BLOCK] + tile_base[blockIdx.x] + incl - c;
  for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) before += wsum[w];
  while (m) {
    const uint32_t j = (uint32_t)__builtin_ctz(m);
    m &= m - 1u;
    if (before < cap_lines) line_end[before] = at + j;
    ++before;
  }
}

// One thread per record (grid-stride). Line i of the chunk ends at line_end[i]; a last line without '\n' ends at the text's
// end when the chunk is the file's last.
__global__ void __launch_bounds__(256) gmx_records_kernel(const uint8_t *text, IngestState *st, const uint32_t *line_end, uint32_t *rec_start,
                                                          uint32_t *rec_len, uint8_t *skip, uint32_t cap_reads) {
  if (st->flags & GMX_INGEST_TOO_MANY_LINES) return;
  const uint32_t lo = st->text_start, hi = lo + st->text_len, n_nl = st->n_lines;
  const uint32_t last_nl_end = n_nl ? line_end[n_nl - 1] + 1u : lo;
  const bool virt = st->final_chunk && last_nl_end < hi;  // text behind the last newline of the file's last chunk: a line
  const uint32_t lines = n_nl + (virt ? 1u : 0u);
  uint32_t n_reads = lines / 4u;
  bool too_many = false;
  if (n_reads > cap_reads) {
    n_reads = 0;
    too_many = true;
  }
  auto le = [&](uint32_t i) { return i < n_nl ? line_end[i] : hi; };
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  unsigned long long bases = 0;
  bool bad = false;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) {
    const uint32_t s1 = r ? line_end[4u * r - 1u] + 1u : lo;
    const uint32_t e1 = le(4u * r), e2 = le(4u * r + 1u), e3 = le(4u * r + 2u), e4 = le(4u * r + 3u);
    const uint32_t s2 = e1 + 1u, s3 = e2 + 1u, s4 = e3 + 1u;
    uint32_t n = e2 - s2, nq = e4 >= s4 ? e4 - s4 : 0u;
    if (n && text[s2 + n - 1u] == '\r') --n;
    if (nq && text[s4 + nq - 1u] == '\r') --nq;
    if (text[s1] != '@' || s3 >= hi || text[s3] != '+' || nq != n || n == 0) bad = true;
    rec_start[r] = s2;
    rec_len[r] = n;
    skip[r] = 0;
    mn = min(mn, n);
    mx = max(mx, n);
    bases += n;
    if (r == n_reads - 1u) {
      const uint32_t end = e4 < hi ? e4 + 1u : hi;
      st->consumed = end;
      st->tail_len = hi - end;
      if (st->final_chunk && end != hi) atomicOr(&st->flags, GMX_INGEST_BAD_RECORD);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->n_reads = n_reads;
    if (too_many) atomicOr(&st->flags, GMX_INGEST_TOO_MANY_LINES);
    if (n_reads == 0) {
      st->consumed = lo;
      st->tail_len = hi - lo;
      if (st->final_chunk && hi != lo) atomicOr(&st->flags, GMX_INGEST_BAD_RECORD);  // fewer than four lines at the end of the file
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_down(mn, off));
    mx = max(mx, (uint32_t)__shfl_down(mx, off));
    bases += __shfl_down(bases, off);
  }
  const unsigned long long any_bad = __ballot(bad);
  if ((threadIdx.x & 63u) == 0) {
    if (mn != 0xFFFFFFFFu) atomicMin(&st->min_len, mn);
    if (mx) atomicMax(&st->max_len, mx);
    if (bases) atomicAdd(&st->n_bases, bases);
    if (any_bad) atomicOr(&st->flags, GMX_INGEST_BAD_RECORD);
  }
}
// one length for all reads? -> layout of the planes; reads of different lengths: their base offsets (one block)
__global__ void __launch_bounds__(64) gmx_layout_kernel(IngestState *st, const IngestInflateStatus *inf) {
  if (threadIdx.x == 0 && inf && inf->flags) {  // what the inflate kernel reported
    st->flags |= inf->flags;
    st->bad_member = inf->bad_member;
  }
  const uint32_t n = st->n_reads;
  const bool uniform = n != 0 && st->min_len == st->max_len;
  if (threadIdx.x == 0) {
    st->uniform_len = uniform ? st->max_len : 0u;
    const unsigned long long ppr = (st->max_len + 31u) / 32u;
    if (uniform || n == 0) st->n_pairs = (unsigned long long)n * ppr;
    for (uint32_t i = 0; i < 16u; ++i) st->sub_pairs[i] = uniform || n == 0 ? ((unsigned long long)i << 20) * ppr : 0ull;
  }
}
// reads of different lengths: their base offsets, offsets[0, n] (two-level scan as above; nothing to do for one length)
__global__ void __launch_bounds__(64) gmx_offsets1_kernel(const IngestState *st, const uint32_t *rec_len, unsigned long long *offsets, unsigned long long *off_blk) {
  const uint32_t n = st->n_reads;
  if (st->uniform_len || blockIdx.x * ING_SCAN_BLOCK >= n) return;
  ing_scan_level1<uint32_t, unsigned long long, unsigned long long>(rec_len, offsets, n, blockIdx.x, off_blk);
}
__global__ void __launch_bounds__(64) gmx_offsets2_kernel(IngestState *st, unsigned long long *offsets, unsigned long long *off_blk) {
  const uint32_t n = st->n_reads;
  if (st->uniform_len || n == 0) return;
  const unsigned long long total = ing_scan_level2<unsigned long long>(off_blk, (n + ING_SCAN_BLOCK - 1u) / ING_SCAN_BLOCK);
  if (threadIdx.x == 0) {
    offsets[n] = total;
    st->n_pairs = (total >> 5) + n;
  }
}
__global__ void __launch_bounds__(64) gmx_offsets3_kernel(IngestState *st, unsigned long long *offsets, const unsigned long long *off_blk) {
  const uint32_t n = st->n_reads;
  if (st->uniform_len || blockIdx.x * ING_SCAN_BLOCK >= n) return;
  const unsigned long long base = off_blk[blockIdx.x];
  const uint32_t at = blockIdx.x * ING_SCAN_BLOCK + (threadIdx.x & 63u) * 16u;
  for (uint32_t j = 0; j < 16u; ++j) {
    const uint32_t r = at + j;
    if (r >= n) break;
    const unsigned long long off = offsets[r] + base;
    offsets[r] = off;
    if ((r & 0xFFFFFu) == 0 && (r >> 20) < 16u) st->sub_pairs[r >> 20] = (off >> 5) + r;  // where a launch of <= 2^20 reads starts
  }
}
// One thread per pair of planes: 32 letters -> (low bits, high bits) of the codes A,C,G,T = 0..3; from the letters' own bits
// (bit 2 of the ASCII code is the code's high bit, bit 1 XOR bit 2 the low one: 'A' 0x41 'C' 0x43 'G' 0x47 'T' 0x54, either case)
__global__ void __launch_bounds__(256) gmx_fq_pack_kernel(const uint8_t *text, IngestState *st, const uint32_t *rec_start, const uint32_t *rec_len,
                                                          const unsigned long long *offsets, unsigned long long *planes, uint8_t *skip) {
  if (st->flags & (GMX_INGEST_TOO_MANY_LINES | GMX_INGEST_BAD_RECORD)) return;
  const uint32_t n_reads = st->n_reads, uniform = st->uniform_len;
  const uint32_t wpr = (st->max_len + 31u) / 32u + (uniform ? 0u : 1u);
  const unsigned long long items = (unsigned long long)n_reads * wpr;
  for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(it / wpr), w = (uint32_t)(it - (unsigned long long)r * wpr);
    const uint32_t len = rec_len[r];
    unsigned long long first, count;
    if (uniform) {
      first = (unsigned long long)r * wpr;
      count = wpr;
    } else {
      const unsigned long long off = offsets[r];
      first = (off >> 5) + r;
      count = ((off + len) >> 5) - (off >> 5) + 1ull;
    }
    if (w >= count) continue;
    uint32_t lo = 0, hi = 0;
    bool ok = true;
    if (w * 32u < len) {
      const uint8_t *src = text + rec_start[r] + w * 32u;
      const uint32_t m = min(32u, len - w * 32u);
      for (uint32_t j = 0; j < m; ++j) {
        const uint32_t c = src[j], u = c & 0xDFu;
        ok = ok && (u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u);
        const uint32_t h = (c >> 2) & 1u;
        hi |= h << j;
        lo |= (((c >> 1) & 1u) ^ h) << j;
      }
    }
    planes[first + w] = (unsigned long long)lo | ((unsigned long long)hi << 32);
    if (!ok) {
      skip[r] = 1;
      st->any_skip = 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// records whose sequence is not one line: FASTA and one-read-per-line text (gmx_ingest_set_format; the rules are those of
// `gram`'s general host reader, SeqReader::next). Behind the same newline kernels:
//   gmx_seq_lines1_kernel   every line classified — does it start a record (a head), how many bases does it add (its bytes minus
//                           the '\n' and ONE '\r' in front of it; a FASTA header adds none) — and both numbers scanned within
//                           blocks of 1024 lines as one 64-bit sum (heads << 32 | bases: a chunk's text stays below 2^32 bytes);
//                           one wavefront per block, no LDS, as the tile scans above
//   gmx_seq_lines2_kernel   the blocks' sums scanned (one wavefront): heads and bases of the chunk, hence its read count
//   gmx_seq_lines3_kernel   line i: bases of the chunk in front of it -> line_base[i]; a head writes its line into rec_line[record]
//   gmx_seq_records_kernel  record r: lines [rec_line[r], rec_line[r + 1]), length = difference of their line_base; where the text
//                           of a record that lies in ONE line starts (ING_MULTI: it does not); what the chunk's records consume
//   gmx_seq_pack_kernel     gmx_fq_pack_kernel, plus: base 32 w of a record of several lines is found by a binary search over the
//                           record's own lines in line_base, and up to 32 letters are gathered across line ends from there
// FASTA: a head is a line whose first byte is '>'; a record is complete when the next head has been seen or the file ends, so a
// chunk consumes up to its LAST head and carries the rest. LINES: a head is a non-empty line and holds its record.
// ------------------------------------------------------------------------------------------------------------------
#define ING_MULTI 0xFFFFFFFFu   // rec_start[r]: the record's bases lie in several lines (a text offset stays below 3 GB + 1 MB + 64)
#define ING_HEAD 0x8000u        // line_rec[i]: the line starts a record (the low bits: records started in front of it within its block)

__device__ __forceinline__ uint32_t ing_seq_lines(const IngestState *st, const uint32_t *line_end) {  // lines of the chunk, as gmx_records_kernel counts them
  const uint32_t lo = st->text_start, hi = lo + st->text_len, n_nl = st->n_lines;
  const uint32_t last_nl_end = n_nl ? line_end[n_nl - 1] + 1u : lo;
  return n_nl + (st->final_chunk && last_nl_end < hi ? 1u : 0u);
}
__device__ __forceinline__ uint32_t ing_seq_line_start(const uint32_t *line_end, uint32_t i, uint32_t lo) { return i ? line_end[i - 1u] + 1u : lo; }

__global__ void __launch_bounds__(64) gmx_seq_lines1_kernel(const uint8_t *text, IngestState *st, const uint32_t *line_end, uint32_t format, uint16_t *line_rec,
                                                            uint32_t *line_base, unsigned long long *blk_tot) {
  if (st->flags & GMX_INGEST_TOO_MANY_LINES) return;
  const uint32_t lines = ing_seq_lines(st, line_end);
  if (blockIdx.x * ING_SCAN_BLOCK >= lines) return;
  const uint32_t lo = st->text_start, hi = lo + st->text_len, n_nl = st->n_lines;
  const uint32_t lane = threadIdx.x & 63u, base = blockIdx.x * ING_SCAN_BLOCK + lane * 16u;
  unsigned long long v[16], sum = 0;
  bool bad = false;
  uint32_t s = base < lines ? ing_seq_line_start(line_end, base, lo) : 0u;
#pragma unroll
  for (uint32_t j = 0; j < 16u; ++j) {
    v[j] = 0;
    if (base + j < lines) {
      const uint32_t e = base + j < n_nl ? line_end[base + j] : hi;
      uint32_t n = e - s;
      const uint32_t first = n ? text[s] : 0u;
      if (n && text[e - 1u] == '\r') --n;
      if (format == GMX_INGEST_FORMAT_FASTA) {
        v[j] = first == '>' ? 1ull << 32 : (unsigned long long)n;
      } else if (n) {
        v[j] = (1ull << 32) | n;
        bad = bad || first == '@' || first == '>';  // (the host reader changes format there)
      }
      s = e + 1u;
    }
    sum += v[j];
  }
  unsigned long long incl = sum;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = __shfl_up(incl, d);
    if ((int)lane >= d) incl += up;
  }
  unsigned long long run = incl - sum;
#pragma unroll
  for (uint32_t j = 0; j < 16u; ++j) {
    if (base + j < lines) {
      line_rec[base + j] = (uint16_t)((uint32_t)(run >> 32) | (v[j] >> 32 ? ING_HEAD : 0u));
      line_base[base + j] = (uint32_t)run;
    }
    run += v[j];
  }
  if (lane == 63u) blk_tot[blockIdx.x] = incl;
  const unsigned long long any_bad = __ballot(bad);
  if (lane == 0 && any_bad) atomicOr(&st->flags, GMX_INGEST_BAD_RECORD);
}
__global__ void __launch_bounds__(64) gmx_seq_lines2_kernel(IngestState *st, const uint32_t *line_end, uint32_t format, unsigned long long *blk_tot, uint32_t *line_base,
                                                            uint32_t *rec_line, uint32_t cap_reads) {
  if (st->flags & GMX_INGEST_TOO_MANY_LINES) return;
  const uint32_t lines = ing_seq_lines(st, line_end);
  const unsigned long long total = ing_scan_level2<unsigned long long>(blk_tot, (lines + ING_SCAN_BLOCK - 1u) / ING_SCAN_BLOCK);
  if (threadIdx.x == 0) {
    const uint32_t heads = (uint32_t)(total >> 32);
    // FASTA: the last head's record goes on in the next chunk unless this one is the file's last
    uint32_t n_reads = format == GMX_INGEST_FORMAT_FASTA && !st->final_chunk ? (heads ? heads - 1u : 0u) : heads;
    if (n_reads > cap_reads) {
      n_reads = 0;
      atomicOr(&st->flags, GMX_INGEST_TOO_MANY_LINES);
    } else {
      line_base[lines] = (uint32_t)total;  // (the arrays have room for cap_lines + 2 lines and cap_reads + 2 records)
      rec_line[heads] = lines;
    }
    st->n_heads = heads;
    st->n_reads = n_reads;
  }
}
__global__ void __launch_bounds__(256) gmx_seq_lines3_kernel(const IngestState *st, const uint32_t *line_end, const uint16_t *line_rec, uint32_t *line_base,
                                                             const unsigned long long *blk_tot, uint32_t *rec_line) {
  if (st->flags & GMX_INGEST_TOO_MANY_LINES) return;
  const uint32_t lines = ing_seq_lines(st, line_end);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < lines; i += gridDim.x * blockDim.x) {
    const unsigned long long t = blk_tot[i / ING_SCAN_BLOCK];
    const uint32_t lr = line_rec[i];
    line_base[i] += (uint32_t)t;
    if (lr & ING_HEAD) rec_line[(uint32_t)(t >> 32) + (lr & (ING_HEAD - 1u))] = i;  // (at most n_heads - 1 <= cap_reads)
  }
}
__global__ void __launch_bounds__(256) gmx_seq_records_kernel(IngestState *st, const uint32_t *line_end, uint32_t format, const uint32_t *line_base,
                                                              const uint32_t *rec_line, uint32_t *rec_start, uint32_t *rec_len, uint8_t *skip) {
  if (st->flags & GMX_INGEST_TOO_MANY_LINES) return;
  const uint32_t lo = st->text_start, hi = lo + st->text_len, n_nl = st->n_lines, n_reads = st->n_reads, heads = st->n_heads;
  const bool fasta = format == GMX_INGEST_FORMAT_FASTA;
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  unsigned long long bases = 0;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += gridDim.x * blockDim.x) {
    const uint32_t l0 = rec_line[r], l1 = rec_line[r + 1u], b0 = line_base[l0];
    const uint32_t len = line_base[l1] - b0;
    const uint32_t j = fasta ? l0 + 1u : l0;  // the first line that may hold bases
    const bool one_line = len == 0 || line_base[j + 1u] - line_base[j] == len;
    rec_start[r] = !one_line ? ING_MULTI : len ? ing_seq_line_start(line_end, j, lo) : lo;
    rec_len[r] = len;
    skip[r] = 0;
    mn = min(mn, len);
    mx = max(mx, len);
    bases += len;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t lines = ing_seq_lines(st, line_end);
    // FASTA: bases in front of the first head belong to no record (the host reader would take the file for one read per line)
    if (fasta && (heads ? line_base[rec_line[0]] : line_base[lines]) != 0) atomicOr(&st->flags, GMX_INGEST_BAD_RECORD);
    uint32_t end = hi;
    if (!st->final_chunk) end = fasta ? (heads ? ing_seq_line_start(line_end, rec_line[heads - 1u], lo) : lo) : (n_nl ? line_end[n_nl - 1u] + 1u : lo);
    st->consumed = end;
    st->tail_len = hi - end;
  }
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_down(mn, off));
    mx = max(mx, (uint32_t)__shfl_down(mx, off));
    bases += __shfl_down(bases, off);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (mn != 0xFFFFFFFFu) atomicMin(&st->min_len, mn);
    if (mx) atomicMax(&st->max_len, mx);
    if (bases) atomicAdd(&st->n_bases, bases);
  }
}
// letters src[0, m) -> bits [at, at + m) of a pair of planes (the arithmetic of gmx_fq_pack_kernel)
__device__ __forceinline__ void ing_pack_letters(const uint8_t *src, uint32_t m, uint32_t at, uint32_t &lo, uint32_t &hi, bool &ok) {
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t c = src[j], u = c & 0xDFu;
    ok = ok && (u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u);
    const uint32_t h = (c >> 2) & 1u;
    hi |= h << (at + j);
    lo |= (((c >> 1) & 1u) ^ h) << (at + j);
  }
}
__global__ void __launch_bounds__(256) gmx_seq_pack_kernel(const uint8_t *text, IngestState *st, const uint32_t *line_end, const uint32_t *line_base,
                                                           const uint32_t *rec_line, const uint32_t *rec_start, const uint32_t *rec_len,
                                                           const unsigned long long *offsets, unsigned long long *planes, uint8_t *skip) {
  if (st->flags & (GMX_INGEST_TOO_MANY_LINES | GMX_INGEST_BAD_RECORD)) return;
  const uint32_t n_reads = st->n_reads, uniform = st->uniform_len, text_lo = st->text_start;
  const uint32_t wpr = (st->max_len + 31u) / 32u + (uniform ? 0u : 1u);
  const unsigned long long items = (unsigned long long)n_reads * wpr;
  for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(it / wpr), w = (uint32_t)(it - (unsigned long long)r * wpr);
    const uint32_t len = rec_len[r];
    unsigned long long first, count;
    if (uniform) {
      first = (unsigned long long)r * wpr;
      count = wpr;
    } else {
      const unsigned long long off = offsets[r];
      first = (off >> 5) + r;
      count = ((off + len) >> 5) - (off >> 5) + 1ull;
    }
    if (w >= count) continue;
    uint32_t lo = 0, hi = 0;
    bool ok = true;
    if (w * 32u < len) {
      const uint32_t m = min(32u, len - w * 32u), start = rec_start[r];
      if (start != ING_MULTI) {
        ing_pack_letters(text + start + w * 32u, m, 0u, lo, hi, ok);
      } else {
        uint32_t a = rec_line[r], b = rec_line[r + 1u];
        const uint32_t target = line_base[a] + w * 32u;  // the base wanted, counted over the chunk: in the last line of [a, b) that starts at or in front of it
        while (b - a > 1u) {
          const uint32_t mid = a + (b - a) / 2u;
          if (line_base[mid] <= target) a = mid;
          else b = mid;
        }
        uint32_t at_base = line_base[a], within = target - at_base;
        for (uint32_t got = 0; got < m; ++a) {  // (bases are left, so lines of the record are: a stays below rec_line[r + 1])
          const uint32_t next_base = line_base[a + 1u];
          const uint32_t take = min(m - got, next_base - at_base - within);
          if (take) ing_pack_letters(text + ing_seq_line_start(line_end, a, text_lo) + within, take, got, lo, hi, ok);
          got += take;
          within = 0;
          at_base = next_base;
        }
      }
    }
    planes[first + w] = (unsigned long long)lo | ((unsigned long long)hi << 32);
    if (!ok) {
      skip[r] = 1;
      st->any_skip = 1;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// BAM (GMX_INGEST_FORMAT_BAM; include/gmx.h has the record layout and the rules): binary records, each found only through the
// block_size of the record before it. In place of the newline and record kernels, speculate / link / repair as
// gmx_gz_link_kernel does for plain gzip:
//   gmx_bam_chain_kernel    the text cut into TILES (GMX_BAM_TILE bytes, 4 KB by default). One wavefront per tile looks for the
//                           first position in the tile that could start a record (64 positions a step, bam_plausible) and walks
//                           the block_size links from there to the first record start at or past the tile's end: the starts it
//                           passed, their count, where it left the tile. The tile that holds the chunk's entry — the header's end
//                           or the carried record's start — starts there without a search.
//   gmx_bam_link_kernel     one wavefront compares every tile's guess with the exit of the tile before, 256 tiles a step. A tile
//                           whose guess is not its true entry is walked again from the true entry (gmx_ingest_bam_rewalks). The
//                           chunk's records end where the walk meets the text's end or a malformed record.
//   gmx_bam_scan1/2_kernel  the tiles' record counts -> where each tile's records go; the chunk's read count
//   gmx_bam_records_kernel  record r: where its seq starts, l_seq, the strand; min / max / sum of the lengths
//   gmx_bam_pack_kernel     32 bases -> a pair of planes from 16 bytes of 4-bit codes; a reverse-strand read from the mirrored
//                           position, complemented
// INVARIANT: a record is accepted only in a tile whose walk started at the tile's TRUE entry, and tile 0's true entry is given:
// every accepted record is reached from the file's first by block_size links alone. bam_plausible only chooses where a
// speculative walk starts; whatever it accepts or misses, the reads are those of the serial walk.
// ------------------------------------------------------------------------------------------------------------------
#define BAM_NONE 0xFFFFFFFFu  // a tile's guess: no position in it could start a record
#define BAM_T_BAD 1u          // a tile's walk stopped at a malformed record
#define BAM_T_OVER 2u         // ... at more starts than a tile has room for (records of >= 37 bytes: cannot happen)
#define BAM_REC_MIN 37u       // block_size (4) + fixed fields (32) + a name of one byte

struct BamArgs {
  const uint8_t *text;
  IngestState *st;
  uint32_t *guess, *exit, *count, *flag, *starts;  // per tile; starts: `room` positions per tile
  uint32_t n_tiles, tile, room;
  uint32_t header_skip;   // bytes of the BAM header at the start of this chunk's members' text
  uint32_t header_left;   // bytes of header the file's text still owes behind this chunk (a final chunk: truncated)
  uint32_t *rewalks;
};

__device__ __forceinline__ uint32_t bam_ld32(const uint8_t *text, uint32_t at) {  // little-endian, any alignment (the buffer is padded)
  const uint32_t *w = reinterpret_cast<const uint32_t *>(text + (at & ~3u));
  return __funnelshift_r(w[0], w[1], (at & 3u) * 8u);
}
__device__ __forceinline__ uint32_t bam_ld16(const uint8_t *text, uint32_t at) { return (uint32_t)text[at] | (uint32_t)text[at + 1u] << 8; }

// the tile's span of the slot's text buffer: tile 0 also holds what was carried in front of the members' text
__device__ __forceinline__ void bam_span(const BamArgs &a, uint32_t t, uint32_t entry, uint32_t hi, uint32_t &lo_t, uint32_t &b_t) {
  const unsigned long long nominal = (unsigned long long)ING_CARRY_MAX + (unsigned long long)t * a.tile;
  lo_t = max(entry, t ? (uint32_t)min(nominal, (unsigned long long)hi) : 0u);
  b_t = (uint32_t)min(nominal + a.tile, (unsigned long long)hi);
}
__device__ __forceinline__ uint32_t bam_entry(const BamArgs &a) { return a.st->text_start + a.header_skip; }

// the malformed-record test of include/gmx.h on the record at p, whose 36 leading bytes lie in the text
__device__ __forceinline__ bool bam_malformed(const uint8_t *text, uint32_t p, uint32_t bs) {
  const uint32_t l_name = text[p + 12u], n_cigar = bam_ld16(text, p + 16u);
  const int32_t l_seq = (int32_t)bam_ld32(text, p + 20u);
  if (l_name == 0 || l_seq < 0) return true;
  const unsigned long long need = 32ull + l_name + 4ull * n_cigar + ((unsigned long long)l_seq + 1ull) / 2ull + (unsigned long long)l_seq;
  return (unsigned long long)bs < need;
}
// could a record start at p? (chooses where a speculative walk starts, nothing else)
__device__ __forceinline__ bool bam_plausible1(const uint8_t *text, uint32_t p, uint32_t hi, uint32_t &bs) {
  if (hi - p < 36u) return false;
  bs = bam_ld32(text, p);
  if (bs < BAM_REC_MIN - 4u || bs > (1u << 28)) return false;
  if ((int32_t)bam_ld32(text, p + 4u) < -1 || (int32_t)bam_ld32(text, p + 24u) < -1) return false;  // refID, next_refID
  if (bam_malformed(text, p, bs)) return false;
  const uint32_t name_end = p + 36u + text[p + 12u] - 1u;
  return name_end >= hi || text[name_end] == 0;
}
// ... and where it ends, the text's end or another one? The fields alone pass at 1.5 places per record of 150 bases that are
// none (quality bytes taken for a block_size of some 2^25 in front of the next record's fields: two tiles of three guessed
// wrong, profiles/bam_device); with the successor, none in 4 M records. The record the chunk's end cuts is not plausible: the
// tile behind the last complete one finds no guess and is entered again by the link kernel, once a chunk.
__device__ __forceinline__ bool bam_plausible(const uint8_t *text, uint32_t p, uint32_t hi) {
  uint32_t bs, bs2;
  if (!bam_plausible1(text, p, hi, bs)) return false;
  if (bs > hi - p - 4u) return false;
  const uint32_t q = p + 4u + bs;  // (<= hi)
  return hi - q < 36u || bam_plausible1(text, q, hi, bs2);
}

struct BamWalk {
  uint32_t exit, count, flag;
};
// Wave-uniform: the chain of block_size links from p to the first record start at or past b; stops in front of a record the text
// cuts (exit < b, no flag) or a malformed one (BAM_T_BAD). Lane 0 writes the starts passed.
__device__ __forceinline__ BamWalk bam_walk(const uint8_t *text, uint32_t p, uint32_t b, uint32_t hi, uint32_t *starts, uint32_t room, bool lane0) {
  BamWalk w{p, 0u, 0u};
  while (w.exit < b) {
    const uint32_t at = w.exit;
    if (hi - at < 4u) break;
    const uint32_t bs = uni(bam_ld32(text, at));
    if ((int32_t)bs < (int32_t)(BAM_REC_MIN - 4u)) {
      w.flag = BAM_T_BAD;
      break;
    }
    if (hi - at >= 36u && uni(bam_malformed(text, at, bs) ? 1u : 0u)) {
      w.flag = BAM_T_BAD;
      break;
    }
    if (bs > hi - at - 4u) break;  // the text ends inside the record
    if (w.count >= room) {
      w.flag = BAM_T_OVER;
      break;
    }
    if (lane0) starts[w.count] = at;
    ++w.count;
    w.exit = at + 4u + bs;
  }
  return w;
}

__global__ void __launch_bounds__(64) gmx_bam_chain_kernel(BamArgs a) {
  const uint32_t t = blockIdx.x, lane = threadIdx.x & 63u;
  const uint32_t hi = a.st->text_start + a.st->text_len, entry = min(bam_entry(a), hi);
  uint32_t lo_t, b_t;
  bam_span(a, t, entry, hi, lo_t, b_t);
  uint32_t guess = BAM_NONE;
  if (lo_t >= b_t) {  // in front of the entry (header), or nothing left: no record starts here
    if (lane == 0) {
      a.guess[t] = a.exit[t] = entry;
      a.count[t] = a.flag[t] = 0;
    }
    return;
  }
  if (lo_t == entry) {
    guess = entry;
  } else {
    for (uint32_t at = lo_t; at < b_t && guess == BAM_NONE; at += 64u) {
      const uint32_t p = at + lane;
      const unsigned long long hit = __ballot(p < b_t && bam_plausible(a.text, p, hi));
      if (hit) guess = at + (uint32_t)__builtin_ctzll(hit);
    }
  }
  BamWalk w{BAM_NONE, 0u, 0u};
  if (guess != BAM_NONE) w = bam_walk(a.text, guess, b_t, hi, a.starts + (size_t)t * a.room, a.room, lane == 0);
  if (lane == 0) {
    a.guess[t] = guess;
    a.exit[t] = w.exit;
    a.count[t] = w.count;
    a.flag[t] = w.flag;
  }
}

__global__ void __launch_bounds__(64) gmx_bam_link_kernel(BamArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  IngestState *const st = a.st;
  const uint32_t hi = uni(st->text_start) + uni(st->text_len), entry = min(bam_entry(a), hi);
  uint32_t prev_exit = entry, last_flag = 0, n_valid = a.n_tiles, rewalks = 0;
  bool ended = false, last_known = false;  // last_known: last_flag is that of the last tile taken
  for (uint32_t t = 0; t < a.n_tiles && !ended;) {
    // tiles [t, t + 256): whose guess is not the exit of the tile before? (lane 0 of the first round: the exit known here)
    uint32_t first_bad = BAM_NONE;
    const uint32_t span = min(256u, a.n_tiles - t);
    for (uint32_t k = 0; k < span && first_bad == BAM_NONE; k += 64u) {
      const uint32_t j = t + k + lane;
      bool ok = true;
      if (k + lane < span) {
        const uint32_t g = a.guess[j], pe = (k + lane) ? a.exit[j - 1u] : prev_exit;
        ok = g != BAM_NONE && g == pe;
      }
      const unsigned long long bad = __ballot(!ok);
      if (bad) first_bad = t + k + (uint32_t)__builtin_ctzll(bad);
    }
    if (first_bad == BAM_NONE) {
      t += span;
      prev_exit = uni(a.exit[t - 1u]);
      last_known = false;
      continue;
    }
    const uint32_t j = first_bad;
    if (j > t) prev_exit = uni(a.exit[j - 1u]);
    uint32_t lo_j, b_j;
    bam_span(a, j, entry, hi, lo_j, b_j);
    BamWalk w{prev_exit, 0u, 0u};
    if (prev_exit < b_j) {  // the tile again, from its true entry
      w = bam_walk(a.text, prev_exit, b_j, hi, a.starts + (size_t)j * a.room, a.room, lane == 0);
      if (w.count) ++rewalks;  // (not the walk that only meets the record the chunk's end cuts: no guess was wrong there)
    }
    if (lane == 0) {
      a.guess[j] = prev_exit;
      a.exit[j] = w.exit;
      a.count[j] = w.count;
      a.flag[j] = w.flag;
    }
    prev_exit = w.exit;
    last_flag = w.flag;
    last_known = true;
    t = j + 1u;
    if (w.exit < b_j) {  // the text's end inside a record, or a malformed one: the chunk's records end here
      ended = true;
      n_valid = t;
    }
  }
  if (!last_known) last_flag = uni(a.flag[n_valid - 1u]);
  if (lane == 0) {
    uint32_t flags = 0;
    if (last_flag & BAM_T_BAD) flags |= GMX_INGEST_BAD_RECORD;
    if (last_flag & BAM_T_OVER) flags |= GMX_INGEST_TOO_MANY_LINES;
    if (st->final_chunk && (prev_exit != hi || a.header_left)) flags |= GMX_INGEST_BAD_RECORD;  // the file ends inside a record, or inside its header
    if (flags) atomicOr(&st->flags, flags);
    st->n_lines = n_valid;  // (tiles whose records count: gmx_bam_scan1/2_kernel, gmx_bam_records_kernel)
    st->consumed = prev_exit;
    st->tail_len = hi - prev_exit;
    if (rewalks) atomicAdd(a.rewalks, rewalks);
  }
}

__global__ void __launch_bounds__(64) gmx_bam_scan1_kernel(BamArgs a, uint32_t *tile_blk) {
  ing_scan_level1<uint32_t, uint32_t, uint32_t>(a.count, a.count, a.st->n_lines, blockIdx.x, tile_blk);
}
__global__ void __launch_bounds__(64) gmx_bam_scan2_kernel(uint32_t *tile_blk, uint32_t n_blk, IngestState *st, uint32_t cap_reads) {
  const uint32_t total = ing_scan_level2<uint32_t>(tile_blk, n_blk);  // (records of >= 37 bytes in < 2^32 bytes of text: fits)
  if (threadIdx.x == 0) {
    if (total > cap_reads) {
      atomicOr(&st->flags, GMX_INGEST_TOO_MANY_LINES);
      st->n_reads = 0;
    } else {
      st->n_reads = total;
    }
  }
}
// One thread per (tile, place in the tile): the record's fixed fields -> where its seq starts, l_seq, the strand.
__global__ void __launch_bounds__(256) gmx_bam_records_kernel(BamArgs a, const uint32_t *tile_base, const uint32_t *tile_blk, uint32_t *rec_start, uint32_t *rec_len,
                                                              uint8_t *rev, uint8_t *skip) {
  IngestState *const st = a.st;
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  unsigned long long bases = 0;
  if (!(st->flags & GMX_INGEST_TOO_MANY_LINES)) {
    const unsigned long long items = (unsigned long long)st->n_lines * a.room;
    for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
      const uint32_t t = (uint32_t)(it / a.room), k = (uint32_t)(it - (unsigned long long)t * a.room);
      const uint32_t base = tile_base[t], next = t + 1u < st->n_lines ? tile_base[t + 1u] + tile_blk[(t + 1u) / ING_SCAN_BLOCK] : st->n_reads;
      const uint32_t r = base + tile_blk[t / ING_SCAN_BLOCK] + k;
      if (r >= next) continue;  // (the tile holds next - first records)
      const uint32_t p = a.starts[(size_t)t * a.room + k];
      const uint32_t l_name = a.text[p + 12u], n_cigar = bam_ld16(a.text, p + 16u), flag = bam_ld16(a.text, p + 18u), l_seq = bam_ld32(a.text, p + 20u);
      rec_start[r] = p + 36u + l_name + 4u * n_cigar;
      rec_len[r] = l_seq;
      rev[r] = (flag & 0x10u) ? 1 : 0;
      skip[r] = 0;
      mn = min(mn, l_seq);
      mx = max(mx, l_seq);
      bases += l_seq;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    mn = min(mn, (uint32_t)__shfl_down(mn, off));
    mx = max(mx, (uint32_t)__shfl_down(mx, off));
    bases += __shfl_down(bases, off);
  }
  if ((threadIdx.x & 63u) == 0) {
    if (mn != 0xFFFFFFFFu) atomicMin(&st->min_len, mn);
    if (mx) atomicMax(&st->max_len, mx);
    if (bases) atomicAdd(&st->n_bases, bases);
  }
}

// eight 4-bit codes of a word, code k in bits [4k, 4k + 4): bit k of the result = bit `which` of code k
__device__ __forceinline__ uint32_t bam_gather(uint32_t x) {  // x: a bit at 0, 4, 8, ..., 28 -> bits 0..7
  x = (x | (x >> 3)) & 0x03030303u;
  x = (x | (x >> 6)) & 0x000F000Fu;
  return (x | (x >> 12)) & 0xFFu;
}
// One thread per pair of planes, as gmx_fq_pack_kernel: 32 bases from 16 bytes of seq (17 when a reverse-strand read's mirrored
// window starts on an odd base). Codes 1, 2, 4, 8 = A, C, G, T -> 0..3: the low plane's bit is "C or T" (code & 0xA), the high
// plane's "G or T" (code & 0xC); any other code (not exactly one bit) flags the read. Reverse strand: read base i is the
// complement of stored base len - 1 - i, and the complement of a 4-bit code is the code with its bits in reverse order
// (A 1 <-> T 8, C 2 <-> G 4; every other code stays a code that flags the read, which is all that is kept of it) — so the
// mirrored, complemented window is the stored window BIT-reversed.
__global__ void __launch_bounds__(256) gmx_bam_pack_kernel(const uint8_t *text, IngestState *st, const uint32_t *rec_start, const uint32_t *rec_len, const uint8_t *rev,
                                                           const unsigned long long *offsets, unsigned long long *planes, uint8_t *skip) {
  if (st->flags & (GMX_INGEST_TOO_MANY_LINES | GMX_INGEST_BAD_RECORD)) return;
  const uint32_t n_reads = st->n_reads, uniform = st->uniform_len;
  const uint32_t wpr = (st->max_len + 31u) / 32u + (uniform ? 0u : 1u);
  const unsigned long long items = (unsigned long long)n_reads * wpr;
  for (unsigned long long it = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (unsigned long long)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(it / wpr), w = (uint32_t)(it - (unsigned long long)r * wpr);
    const uint32_t len = rec_len[r];
    unsigned long long first, count;
    if (uniform) {
      first = (unsigned long long)r * wpr;
      count = wpr;
    } else {
      const unsigned long long off = offsets[r];
      first = (off >> 5) + r;
      count = ((off + len) >> 5) - (off >> 5) + 1ull;
    }
    if (w >= count) continue;
    uint32_t lo = 0, hi = 0;
    bool ok = true;
    if (w * 32u < len) {
      const uint32_t m = min(32u, len - w * 32u);
      const bool reverse = rev[r] != 0;
      // the window of 32 stored bases [s, s + 32): forward the read's own; reverse the mirror image's (s may lie in front of the
      // seq when fewer than 32 bases are left: those codes are masked out below; the bytes are the record's own, cigar or name)
      const long long s = reverse ? (long long)len - 32ll - 32ll * w : 32ll * w;
      const uint32_t byte0 = (uint32_t)((long long)rec_start[r] + (s >> 1));  // (arithmetic shift: floor)
      const bool odd = (s & 1ll) != 0;
      const uint32_t *al = reinterpret_cast<const uint32_t *>(text + (byte0 & ~3u));
      const uint32_t sh = (byte0 & 3u) * 8u;
      uint32_t x[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const uint32_t v = __funnelshift_r(al[q], al[q + 1], sh);
        x[q] = ((v & 0x0F0F0F0Fu) << 4) | ((v >> 4) & 0x0F0F0F0Fu);  // a byte's HIGH nibble is the earlier base: code k in bits [4k, 4k + 4)
      }
      uint32_t y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = odd ? (x[q] >> 4) | (x[q + 1] << 28) : x[q];
      if (reverse) {
        const uint32_t z0 = __brev(y[3]), z1 = __brev(y[2]), z2 = __brev(y[1]), z3 = __brev(y[0]);
        y[0] = z0, y[1] = z1, y[2] = z2, y[3] = z3;
      }
      uint32_t wrong = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t left = m > 8u * q ? min(8u, m - 8u * q) : 0u;  // codes of this word that are bases of the read
        const uint32_t mask = left == 8u ? 0xFFFFFFFFu : (1u << (4u * left)) - 1u;
        const uint32_t v = y[q] & mask;
        const uint32_t pairs = (v & 0x55555555u) + ((v >> 1) & 0x55555555u);
        const uint32_t ones = (pairs & 0x33333333u) + ((pairs >> 2) & 0x33333333u);  // bits set, per code
        wrong |= (ones ^ 0x11111111u) & mask;
        lo |= bam_gather(((v >> 1) | (v >> 3)) & 0x11111111u) << (8 * q);
        hi |= bam_gather(((v >> 2) | (v >> 3)) & 0x11111111u) << (8 * q);
      }
      ok = wrong == 0;
    }
    planes[first + w] = (unsigned long long)lo | ((unsigned long long)hi << 32);
    if (!ok) {
      skip[r] = 1;
      st->any_skip = 1;
    }
  }
}

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

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
#define GMX_INGEST_SLOTS 3  // chunks in flight per ingest (include/gmx.h: slots 0, 1, 2; a caller may alternate between two of them)
struct gmx_ingest {
  int device = 0;
  uint64_t max_text = 0, max_comp = 0;
  uint32_t cap_reads = 0, cap_lines = 0, cap_members = 0, n_tiles_max = 0;
  hipStream_t stream = nullptr, copy_stream = nullptr;
  struct Slot {
    uint32_t *d_comp = nullptr;
    IngestMember *d_members = nullptr;
    uint8_t *d_text = nullptr;
    uint32_t *d_line_end = nullptr, *d_rec_start = nullptr, *d_rec_len = nullptr, *d_tiles = nullptr, *d_tile_blk = nullptr;
    unsigned long long *d_off_blk = nullptr;  // (the scans' block sums: gmx_tile_scan1/2_kernel, gmx_offsets1/2/3_kernel)
    unsigned long long *d_planes = nullptr, *d_offsets = nullptr;
    uint8_t *d_skip = nullptr;
    // FASTA / LINES (allocated by the first gmx_ingest_set_format that asks for one of them): per line, per record, per 1024 lines
    uint16_t *d_line_rec = nullptr;
    uint32_t *d_line_base = nullptr, *d_rec_line = nullptr;
    unsigned long long *d_line_blk = nullptr;
    // BAM (allocated by the first gmx_ingest_set_format that asks for it): per tile, per place in a tile, per record
    uint32_t *d_bam_guess = nullptr, *d_bam_exit = nullptr, *d_bam_count = nullptr, *d_bam_flag = nullptr, *d_bam_starts = nullptr, *d_bam_blk = nullptr;
    uint8_t *d_bam_rev = nullptr;
    IngestState *d_state = nullptr, *h_state = nullptr;
    IngestMember *h_members = nullptr;  // page-locked staging of the member table
    IngestInflateStatus *d_inflate_status = nullptr;
    hipStream_t inflate_stream = nullptr;  // the slot's inflate kernel: beside the scan of the chunk before and the tail of its inflate kernel
    hipEvent_t copied = nullptr, done = nullptr, released = nullptr, released2 = nullptr, inflated = nullptr, carried = nullptr;
    bool in_flight = false, has_release = false, has_release2 = false, has_carried = false;
    hipEvent_t follower_carried = nullptr;  // `carried` of the chunk that continued this slot's: its carry kernel read the end of this slot's text
    bool has_follower = false;
    bool deferred = false;       // gmx_ingest_submit_bgzf_deferred / _text_deferred: uploaded (and inflating), scan still to come (gmx_ingest_scan)
    bool deferred_inflate = true;  // ... with an inflate kernel (false: the chunk arrived as text)
    uint32_t deferred_text = 0;  // ... bytes of text of its members
  } slot[GMX_INGEST_SLOTS];
  int last_slot = -1;  // the slot whose chunk the next one continues (-1: a file's first chunk)
  int format = GMX_INGEST_FORMAT_FASTQ;  // gmx_ingest_set_format
  std::vector<void *> allocs;
  int check_crc = 1;
  uint32_t exp_mode = 0;
  unsigned long long *d_dbg = nullptr;  // GMX_INGEST_STATS=1: counters of gmx_inflate_kernel, printed by gmx_ingest_destroy
  struct Gz {  // plain gzip (gmx_ingest_submit_gzip): allocated by the first such chunk; used on `stream` only, chunk after chunk
    GzPiece *d_pieces = nullptr;
    uint16_t *d_sym = nullptr;       // max_pieces * cap symbols
    uint8_t *d_wins = nullptr;       // the 32 KB in front of each piece
    uint8_t *d_window = nullptr;     // the last 32 KB of the chunk before
    GzState *d_state = nullptr;
    uint32_t piece_bytes = 0, max_pieces = 0, cap = 0, late_mod = 0, drop_mod = 0;
  } *gz = nullptr;
  bool gz_fresh = true;  // the next gzip chunk starts a file
  // BAM: the tile size (GMX_BAM_TILE, read when the tables are made), tiles and starts per tile the tables hold, header bytes the
  // file's text still owes (gmx_ingest_set_bam_header; the chunks' text lengths are known to the host), the rewalk counter
  uint32_t bam_tile = 0, bam_tiles_max = 0, bam_room = 0;
  uint64_t bam_header_left = 0;
  uint32_t *d_bam_rewalks = nullptr;
};

namespace {
template <class T>
int ing_alloc(gmx_ingest *g, T **p, size_t count, bool zero) {
  void *q = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  ING_TRY(hipMalloc(&q, bytes));
  if (zero) {  // (hipMemset returns before the device is done, and the ingest's streams do not wait for the NULL stream: wait here)
    ING_TRY(hipMemset(q, 0, bytes));
    ING_TRY(hipStreamSynchronize(nullptr));
  }
  g->allocs.push_back(q);
  *p = static_cast<T *>(q);
  return GMX_OK;
}
}  // namespace

extern "C" {

// The slots' inflate streams are created at the LOWEST stream priority: the runtime keeps a pool of hardware queues per priority
// (4 each by default), so the three of them get queues of their own — two streams on one hardware queue run their kernels one after the
// other, and chunk i + 1's inflate kernel then waits for chunk i's instead of filling the CUs its tail leaves idle — without the
// process asking for more queues (GPU_MAX_HW_QUEUES), which changes how an engine's own streams are spread (configs[3]'s host feed
// -12 % at 16). And it is the right order of precedence: scans and mapping kernels go first. GMX_INGEST_STREAM_PRIORITY=0: as the others.
static hipError_t ing_inflate_stream_create(hipStream_t *st) {
  int least = 0, greatest = 0;
  if (getenv("GMX_INGEST_STREAM_PRIORITY") && atoi(getenv("GMX_INGEST_STREAM_PRIORITY")) == 0) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest) {
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  }
  return hipStreamCreateWithPriority(st, hipStreamNonBlocking, least);
}

int gmx_ingest_create(int device, uint64_t max_text_bytes, gmx_ingest **out) try {
  if (!out || max_text_bytes < (1u << 16) || max_text_bytes > (3ull << 30)) {
    gmx_set_error("gmx_ingest_create: max_text_bytes must lie between 64 KB and 3 GB");
    return GMX_EINVAL;
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
    (void)hipGetLastError();
    gmx_set_error("gmx_ingest_create: no such HIP device (reads are decoded on the GPU: there is no CPU fallback here)");
    return GMX_ENODEV;
  }
  ING_TRY(hipSetDevice(device));
  gmx_ingest *g = new gmx_ingest();
  g->device = device;
  g->max_text = max_text_bytes;
  g->max_comp = max_text_bytes / 2 + (1u << 20);
  g->cap_reads = (uint32_t)(max_text_bytes / 32 + 1024);
  g->cap_lines = 4u * g->cap_reads + 8u;
  g->cap_members = (uint32_t)(max_text_bytes / 512 + 1024);  // (members of half a KB of text on average, or larger)
  g->n_tiles_max = (uint32_t)((ING_CARRY_MAX + max_text_bytes + ING_TILE - 1) / ING_TILE);
  g->check_crc = getenv("GMX_INGEST_NO_CRC") ? 0 : 1;
  if (getenv("GMX_INGEST_EXP")) g->exp_mode = (uint32_t)atoi(getenv("GMX_INGEST_EXP"));
  if (getenv("GMX_INGEST_STATS") && ing_alloc(g, &g->d_dbg, 16, true) != GMX_OK) g->d_dbg = nullptr;
  int rc = GMX_OK;
  auto fail = [&](int code) {
    gmx_ingest_destroy(g);
    return code;
  };
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&g->copy_stream, hipStreamNonBlocking) != hipSuccess) {
    gmx_set_error("gmx_ingest_create: hipStreamCreate failed");
    return fail(GMX_EHIP);
  }
  for (auto &s : g->slot) {
    if ((rc = ing_alloc(g, &s.d_comp, g->max_comp / 4 + 256, false)) || (rc = ing_alloc(g, &s.d_members, g->cap_members, false)) ||
        (rc = ing_alloc(g, &s.d_text, ING_CARRY_MAX + max_text_bytes + 64, false)) || (rc = ing_alloc(g, &s.d_line_end, g->cap_lines, false)) ||
        (rc = ing_alloc(g, &s.d_rec_start, g->cap_reads, false)) || (rc = ing_alloc(g, &s.d_rec_len, g->cap_reads, false)) ||
        (rc = ing_alloc(g, &s.d_tiles, g->n_tiles_max + 1, false)) || (rc = ing_alloc(g, &s.d_tile_blk, g->n_tiles_max / ING_SCAN_BLOCK + 2, false)) ||
        (rc = ing_alloc(g, &s.d_off_blk, (size_t)g->cap_reads / ING_SCAN_BLOCK + 2, false)) || (rc = ing_alloc(g, &s.d_planes, max_text_bytes / 16 + 2ull * g->cap_reads + 64, false)) ||
        (rc = ing_alloc(g, &s.d_offsets, (size_t)g->cap_reads + 1, false)) || (rc = ing_alloc(g, &s.d_skip, g->cap_reads, false)) ||
        (rc = ing_alloc(g, &s.d_state, 1, true)) || (rc = ing_alloc(g, &s.d_inflate_status, 1, true)))
      return fail(rc);
    if (hipHostMalloc(reinterpret_cast<void **>(&s.h_state), sizeof(IngestState), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&s.h_members), (size_t)g->cap_members * sizeof(IngestMember), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&s.copied, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess ||
        hipEventCreateWithFlags(&s.released, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&s.released2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.inflated, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.carried, hipEventDisableTiming) != hipSuccess || ing_inflate_stream_create(&s.inflate_stream) != hipSuccess) {
      gmx_set_error("gmx_ingest_create: page-locked memory / events");
      return fail(GMX_EHIP);
    }
  }
  *out = g;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_create")

void gmx_ingest_destroy(gmx_ingest *g) try {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  if (g->copy_stream) (void)hipStreamSynchronize(g->copy_stream);
  if (g->d_dbg) {
    unsigned long long v[16] = {0};
    if (hipMemcpy(v, g->d_dbg, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess && v[10])
      fprintf(stderr, "[gmx_ingest] per member: %.0f look-ups, %.0f literal bytes, %.0f matches (%.0f bytes, %.1f far), %.1f bit-by-bit, %.2f blocks; kclocks %.0f total, %.0f tables, %.0f copies, %.0f crc (%llu members)\n",
              (double)v[0] / v[10], (double)v[1] / v[10], (double)v[2] / v[10], (double)v[11] / v[10], (double)v[3] / v[10], (double)v[4] / v[10], (double)v[5] / v[10],
              v[6] / 1e3 / v[10], v[7] / 1e3 / v[10], v[8] / 1e3 / v[10], v[9] / 1e3 / v[10], v[10]);
  }
  for (auto &s : g->slot) {
    if (s.h_state) (void)hipHostFree(s.h_state);
    if (s.h_members) (void)hipHostFree(s.h_members);
    if (s.copied) (void)hipEventDestroy(s.copied);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.released) (void)hipEventDestroy(s.released);
    if (s.released2) (void)hipEventDestroy(s.released2);
    if (s.inflated) (void)hipEventDestroy(s.inflated);
    if (s.carried) (void)hipEventDestroy(s.carried);
    if (s.inflate_stream) {
      (void)hipStreamSynchronize(s.inflate_stream);
      (void)hipStreamDestroy(s.inflate_stream);
    }
  }
  for (void *p : g->allocs) (void)hipFree(p);
  delete g->gz;
  if (g->stream) (void)hipStreamDestroy(g->stream);
  if (g->copy_stream) (void)hipStreamDestroy(g->copy_stream);
  (void)hipGetLastError();
  delete g;
} GMX_GUARD_VOID("gmx_ingest_destroy")

uint64_t gmx_ingest_max_text(const gmx_ingest *g) { return g ? g->max_text : 0; }
uint64_t gmx_ingest_max_compressed(const gmx_ingest *g) { return g ? g->max_comp : 0; }
uint64_t gmx_ingest_max_members(const gmx_ingest *g) { return g ? g->cap_members : 0; }

int gmx_ingest_set_format(gmx_ingest *g, int format) try {
  if (!g || (format != GMX_INGEST_FORMAT_FASTQ && format != GMX_INGEST_FORMAT_FASTA && format != GMX_INGEST_FORMAT_LINES && format != GMX_INGEST_FORMAT_BAM)) {
    gmx_set_error("gmx_ingest_set_format: null ingest or unknown format");
    return GMX_EINVAL;
  }
  for (const auto &s : g->slot)
    if (s.in_flight || s.deferred) {
      gmx_set_error("gmx_ingest_set_format: a slot's chunk is in flight (the format is set between files)");
      return GMX_EINVAL;
    }
  if (format == GMX_INGEST_FORMAT_BAM && !g->slot[GMX_INGEST_SLOTS - 1].d_bam_rev) {  // the tile tables, once
    ING_TRY(hipSetDevice(g->device));
    uint64_t tile = 4096;
    if (const char *e = getenv("GMX_BAM_TILE")) tile = std::min<uint64_t>(std::max<uint64_t>(64, (uint64_t)atoll(e)), 1u << 20);
    g->bam_tile = (uint32_t)tile;
    g->bam_tiles_max = (uint32_t)((g->max_text + tile - 1) / tile + 1);
    g->bam_room = (uint32_t)(tile / BAM_REC_MIN + 3);  // (records of >= 37 bytes that start in a tile, and the carried one in front of tile 0)
    g->allocs.reserve(g->allocs.size() + 7 * GMX_INGEST_SLOTS + 1);
    int rc;
    if (!g->d_bam_rewalks && (rc = ing_alloc(g, &g->d_bam_rewalks, 1, true))) return rc;
    for (auto &s : g->slot) {
      const size_t n = g->bam_tiles_max;
      if ((!s.d_bam_guess && (rc = ing_alloc(g, &s.d_bam_guess, n, false))) || (!s.d_bam_exit && (rc = ing_alloc(g, &s.d_bam_exit, n, false))) ||
          (!s.d_bam_count && (rc = ing_alloc(g, &s.d_bam_count, n, false))) || (!s.d_bam_flag && (rc = ing_alloc(g, &s.d_bam_flag, n, false))) ||
          (!s.d_bam_starts && (rc = ing_alloc(g, &s.d_bam_starts, n * g->bam_room, false))) ||
          (!s.d_bam_blk && (rc = ing_alloc(g, &s.d_bam_blk, n / ING_SCAN_BLOCK + 2, false))) ||
          (!s.d_bam_rev && (rc = ing_alloc(g, &s.d_bam_rev, g->cap_reads, false))))
        return rc;
    }
  }
  if (format != GMX_INGEST_FORMAT_FASTQ && format != GMX_INGEST_FORMAT_BAM && !g->slot[GMX_INGEST_SLOTS - 1].d_line_blk) {  // the line tables, once
    ING_TRY(hipSetDevice(g->device));
    g->allocs.reserve(g->allocs.size() + 4 * GMX_INGEST_SLOTS);
    for (auto &s : g->slot) {
      int rc;
      if ((!s.d_line_rec && (rc = ing_alloc(g, &s.d_line_rec, (size_t)g->cap_lines + 2, false))) ||
          (!s.d_line_base && (rc = ing_alloc(g, &s.d_line_base, (size_t)g->cap_lines + 2, false))) ||
          (!s.d_rec_line && (rc = ing_alloc(g, &s.d_rec_line, (size_t)g->cap_reads + 2, false))) ||
          (!s.d_line_blk && (rc = ing_alloc(g, &s.d_line_blk, (size_t)g->cap_lines / ING_SCAN_BLOCK + 2, false))))
        return rc;
    }
  }
  g->format = format;
  g->bam_header_left = 0;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_set_format")

int gmx_ingest_set_bam_header(gmx_ingest *g, uint64_t header_bytes) try {
  if (!g || g->format != GMX_INGEST_FORMAT_BAM) {
    gmx_set_error("gmx_ingest_set_bam_header: null ingest, or its format is not GMX_INGEST_FORMAT_BAM");
    return GMX_EINVAL;
  }
  for (const auto &s : g->slot)
    if (s.in_flight || s.deferred) {
      gmx_set_error("gmx_ingest_set_bam_header: a slot's chunk is in flight (the header's length is set in front of a file's first chunk)");
      return GMX_EINVAL;
    }
  g->bam_header_left = header_bytes;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_set_bam_header")

int64_t gmx_ingest_bam_rewalks(gmx_ingest *g) try {
  if (!g) {
    gmx_set_error("null ingest");
    return GMX_EINVAL;
  }
  if (!g->d_bam_rewalks) return 0;
  ING_TRY(hipSetDevice(g->device));
  ING_TRY(hipStreamSynchronize(g->stream));
  uint32_t v = 0;
  ING_TRY(hipMemcpy(&v, g->d_bam_rewalks, 4, hipMemcpyDeviceToHost));
  return (int64_t)v;
} GMX_GUARD_INT("gmx_ingest_bam_rewalks")

int gmx_ingest_reset(gmx_ingest *g) try {  // the next chunk starts a file: nothing is carried into it
  if (!g) {
    gmx_set_error("null ingest");
    return GMX_EINVAL;
  }
  g->last_slot = -1;
  g->gz_fresh = true;
  g->bam_header_left = 0;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_reset")

// The kernels behind a chunk's bytes. Three streams: the slot's own for its inflate kernel — so that it runs beside the scan of
// the chunk before and fills the CUs the tail of that chunk's inflate kernel leaves idle —, one for the scans (in chunk order:
// a chunk's carry needs the state of the chunk before), the copy stream. Orderings that are not a stream's own:
//   inflate(i) after the upload of chunk i, and after carry(i - 1): that kernel reads the END of chunk i - 2's text from this slot
//   scan(i) after inflate(i); the slot's next upload / inflate / pack after whatever read its planes (gmx_ingest_release_after)
static int ing_enqueue_inflate(gmx_ingest *g, int si, uint32_t n_members) {
  gmx_ingest::Slot &s = g->slot[si];
  ING_TRY(hipStreamWaitEvent(s.inflate_stream, s.copied, 0));
  ING_TRY(hipMemsetAsync(&s.d_inflate_status->flags, 0, 4, s.inflate_stream));
  ING_TRY(hipMemsetAsync(&s.d_inflate_status->bad_member, 0xFF, 4, s.inflate_stream));
  if (n_members) {
    if (g->d_dbg)
      hipLaunchKernelGGL(gmx_inflate_kernel<true>, dim3(n_members), dim3(64), 0, s.inflate_stream, s.d_comp, s.d_members, n_members, s.d_text + ING_CARRY_MAX,
                         s.d_inflate_status, g->check_crc, g->d_dbg, g->exp_mode);
    else
      hipLaunchKernelGGL(gmx_inflate_kernel<false>, dim3(n_members), dim3(64), 0, s.inflate_stream, s.d_comp, s.d_members, n_members, s.d_text + ING_CARRY_MAX,
                         s.d_inflate_status, g->check_crc, g->d_dbg, 0u);
  }
  ING_TRY(hipGetLastError());
  ING_TRY(hipEventRecord(s.inflated, s.inflate_stream));
  return GMX_OK;
}
// BAM: the record chain and the pack kernel behind the carry kernel (ing_enqueue_scan; chunks with the cut record on the device only)
static int ing_enqueue_bam(gmx_ingest *g, int si, uint32_t members_text, bool inflate) {
  gmx_ingest::Slot &s = g->slot[si];
  BamArgs a;
  a.text = s.d_text;
  a.st = s.d_state;
  a.guess = s.d_bam_guess;
  a.exit = s.d_bam_exit;
  a.count = s.d_bam_count;
  a.flag = s.d_bam_flag;
  a.starts = s.d_bam_starts;
  a.tile = g->bam_tile;
  a.room = g->bam_room;
  a.n_tiles = (uint32_t)std::max<uint64_t>(1, ((uint64_t)members_text + a.tile - 1) / a.tile);  // (<= bam_tiles_max: members_text <= max_text)
  a.header_skip = (uint32_t)std::min<uint64_t>(g->bam_header_left, members_text);  // (header left: nothing was carried, the chunk before was all header)
  g->bam_header_left -= a.header_skip;
  a.header_left = (uint32_t)std::min<uint64_t>(g->bam_header_left, 0xFFFFFFFFu);
  a.rewalks = g->d_bam_rewalks;
  const uint32_t n_blk = (a.n_tiles + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK;
  hipLaunchKernelGGL(gmx_bam_chain_kernel, dim3(a.n_tiles), dim3(64), 0, g->stream, a);
  hipLaunchKernelGGL(gmx_bam_link_kernel, dim3(1), dim3(64), 0, g->stream, a);
  hipLaunchKernelGGL(gmx_bam_scan1_kernel, dim3(n_blk), dim3(64), 0, g->stream, a, s.d_bam_blk);
  hipLaunchKernelGGL(gmx_bam_scan2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_bam_blk, n_blk, s.d_state, g->cap_reads);
  hipLaunchKernelGGL(gmx_bam_records_kernel, dim3(4096), dim3(256), 0, g->stream, a, (const uint32_t *)s.d_bam_count, (const uint32_t *)s.d_bam_blk, s.d_rec_start,
                     s.d_rec_len, s.d_bam_rev, s.d_skip);
  const uint32_t n_off_blk = (uint32_t)((g->cap_reads + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK);
  hipLaunchKernelGGL(gmx_layout_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, inflate ? s.d_inflate_status : nullptr);
  hipLaunchKernelGGL(gmx_offsets1_kernel, dim3(n_off_blk), dim3(64), 0, g->stream, s.d_state, s.d_rec_len, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_offsets2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_offsets3_kernel, dim3(n_off_blk), dim3(64), 0, g->stream, s.d_state, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_bam_pack_kernel, dim3(4096), dim3(256), 0, g->stream, (const uint8_t *)s.d_text, s.d_state, (const uint32_t *)s.d_rec_start,
                     (const uint32_t *)s.d_rec_len, (const uint8_t *)s.d_bam_rev, (const unsigned long long *)s.d_offsets, s.d_planes, s.d_skip);
  ING_TRY(hipGetLastError());
  ING_TRY(hipMemcpyAsync(s.h_state, s.d_state, sizeof(IngestState), hipMemcpyDeviceToHost, g->stream));
  ING_TRY(hipEventRecord(s.done, g->stream));
  s.in_flight = true;
  s.deferred = false;
  g->last_slot = si;
  return GMX_OK;
}

// host_tail = ~0: the cut record comes from the chunk before on this device (g->last_slot); else that many bytes lie in front of the text
// gz_len: a plain gzip chunk, whose text length the device holds (members_text is then ignored; the newline kernels get a grid
// for max_text, the tiles beyond the text leave at once)
static int ing_enqueue_scan(gmx_ingest *g, int si, uint32_t members_text, int final_chunk, bool inflate, uint32_t n_members, uint32_t host_tail = 0xFFFFFFFFu,
                            const uint32_t *gz_len = nullptr) {
  gmx_ingest::Slot &s = g->slot[si];
  const bool from_device = host_tail == 0xFFFFFFFFu;
  gmx_ingest::Slot *prev = from_device && g->last_slot >= 0 ? &g->slot[g->last_slot] : nullptr;
  if (inflate && from_device) {
    int rc = ing_enqueue_inflate(g, si, n_members);
    if (rc) return rc;
  }
  if (gz_len)
    hipLaunchKernelGGL(gmx_carry_gz_kernel, dim3(64), dim3(256), 0, g->stream, prev ? prev->d_state : nullptr, prev ? prev->d_text : nullptr, s.d_state, s.d_text,
                       gz_len, (uint32_t)(final_chunk ? 1 : 0));
  else
    hipLaunchKernelGGL(gmx_carry_kernel, dim3(64), dim3(256), 0, g->stream, prev ? prev->d_state : nullptr, prev ? prev->d_text : nullptr, s.d_state, s.d_text,
                       members_text, (uint32_t)(final_chunk ? 1 : 0), from_device ? 0u : host_tail);
  ING_TRY(hipEventRecord(s.carried, g->stream));
  s.has_carried = true;
  if (prev) {  // (the slot of the chunk before may be overwritten once this kernel has read its end: ing_begin)
    prev->follower_carried = s.carried;
    prev->has_follower = true;
  }
  ING_TRY(hipStreamWaitEvent(g->stream, inflate ? s.inflated : s.copied, 0));
  if (g->format == GMX_INGEST_FORMAT_BAM) return ing_enqueue_bam(g, si, members_text, inflate);
  const uint32_t n_tiles = gz_len ? g->n_tiles_max : (uint32_t)((ING_CARRY_MAX + (uint64_t)members_text + ING_TILE - 1) / ING_TILE);
  hipLaunchKernelGGL(gmx_nl_count_kernel, dim3(n_tiles), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_tiles);
  const uint32_t n_tile_blk = (n_tiles + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK;
  hipLaunchKernelGGL(gmx_tile_scan1_kernel, dim3(n_tile_blk), dim3(64), 0, g->stream, s.d_tiles, n_tiles, s.d_tile_blk);
  hipLaunchKernelGGL(gmx_tile_scan2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_tile_blk, n_tile_blk, s.d_state, g->cap_lines);
  hipLaunchKernelGGL(gmx_nl_mark_kernel, dim3(n_tiles), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_tiles, s.d_tile_blk, s.d_line_end, g->cap_lines);
  const uint32_t fmt = (uint32_t)g->format;
  if (fmt == GMX_INGEST_FORMAT_FASTQ) {
    hipLaunchKernelGGL(gmx_records_kernel, dim3(2048), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_line_end, s.d_rec_start, s.d_rec_len, s.d_skip, g->cap_reads);
  } else {  // (the chunk's line count is on the device: blocks beyond it leave at once)
    const uint32_t n_line_blk = (uint32_t)(((uint64_t)g->cap_lines + 1 + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK);
    hipLaunchKernelGGL(gmx_seq_lines1_kernel, dim3(n_line_blk), dim3(64), 0, g->stream, s.d_text, s.d_state, s.d_line_end, fmt, s.d_line_rec, s.d_line_base, s.d_line_blk);
    hipLaunchKernelGGL(gmx_seq_lines2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, s.d_line_end, fmt, s.d_line_blk, s.d_line_base, s.d_rec_line, g->cap_reads);
    hipLaunchKernelGGL(gmx_seq_lines3_kernel, dim3(4096), dim3(256), 0, g->stream, s.d_state, s.d_line_end, s.d_line_rec, s.d_line_base, s.d_line_blk, s.d_rec_line);
    hipLaunchKernelGGL(gmx_seq_records_kernel, dim3(2048), dim3(256), 0, g->stream, s.d_state, s.d_line_end, fmt, s.d_line_base, s.d_rec_line, s.d_rec_start, s.d_rec_len, s.d_skip);
  }
  const uint32_t n_off_blk = (uint32_t)((g->cap_reads + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK);  // (the chunk's read count is on the device: blocks beyond it leave at once)
  hipLaunchKernelGGL(gmx_layout_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, inflate || gz_len ? s.d_inflate_status : nullptr);
  hipLaunchKernelGGL(gmx_offsets1_kernel, dim3(n_off_blk), dim3(64), 0, g->stream, s.d_state, s.d_rec_len, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_offsets2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_offsets3_kernel, dim3(n_off_blk), dim3(64), 0, g->stream, s.d_state, s.d_offsets, s.d_off_blk);
  if (fmt == GMX_INGEST_FORMAT_FASTQ)
    hipLaunchKernelGGL(gmx_fq_pack_kernel, dim3(4096), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_rec_start, s.d_rec_len, s.d_offsets, s.d_planes, s.d_skip);
  else
    hipLaunchKernelGGL(gmx_seq_pack_kernel, dim3(4096), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_line_end, s.d_line_base, s.d_rec_line, s.d_rec_start,
                       s.d_rec_len, s.d_offsets, s.d_planes, s.d_skip);
  ING_TRY(hipGetLastError());
  ING_TRY(hipMemcpyAsync(s.h_state, s.d_state, sizeof(IngestState), hipMemcpyDeviceToHost, g->stream));
  ING_TRY(hipEventRecord(s.done, g->stream));
  s.in_flight = true;
  s.deferred = false;
  g->last_slot = from_device ? si : -1;  // (a chunk scanned with a host-provided start carries nothing on the device)
  return GMX_OK;
}

static int ing_not_bam(const char *who) {  // BAM goes through gmx_ingest_submit_bgzf / _submit_text of ONE ingest
  gmx_set_error(std::string(who) + ": not available in GMX_INGEST_FORMAT_BAM (a BAM file's chunks go to one ingest through gmx_ingest_submit_bgzf or gmx_ingest_submit_text)");
  return GMX_EINVAL;
}

static int ing_begin(gmx_ingest *g, int si, const char *who) {
  if (!g || si < 0 || si >= GMX_INGEST_SLOTS) {
    gmx_set_error(std::string(who) + ": null ingest or slot not 0 / 1 / 2");
    return GMX_EINVAL;
  }
  if (g->slot[si].in_flight || g->slot[si].deferred) {
    gmx_set_error(std::string(who) + ": the slot's chunk before has not been waited for (gmx_ingest_wait), or still awaits its gmx_ingest_scan");
    return GMX_EINVAL;
  }
  if (g->last_slot == si) {
    gmx_set_error(std::string(who) + ": the chunk before went to the same slot (the slots alternate: its text holds the start of this chunk's first record; gmx_ingest_reset starts a new file)");
    return GMX_EINVAL;
  }
  ING_TRY(hipSetDevice(g->device));
  gmx_ingest::Slot &s = g->slot[si];
  if (s.has_release) {  // the mapping kernels that read the slot's planes (gmx_ingest_release_after)
    ING_TRY(hipStreamWaitEvent(g->copy_stream, s.released, 0));
    ING_TRY(hipStreamWaitEvent(g->stream, s.released, 0));
    ING_TRY(hipStreamWaitEvent(s.inflate_stream, s.released, 0));
    s.has_release = false;
  }
  if (s.has_release2) {  // (an engine with two workspaces: the launches on its second stream)
    ING_TRY(hipStreamWaitEvent(g->copy_stream, s.released2, 0));
    ING_TRY(hipStreamWaitEvent(g->stream, s.released2, 0));
    ING_TRY(hipStreamWaitEvent(s.inflate_stream, s.released2, 0));
    s.has_release2 = false;
  }
  // this slot's text is about to be overwritten (inflate kernel, or the upload of a text chunk): the carry kernel of the chunk that
  // continued this slot's old chunk reads the end of that text. (With two slots that is the chunk before the one being submitted;
  // with three it ran long ago — the new chunk's inflate kernel does not wait for the scan of the chunk two before it.)
  if (s.has_follower) {
    ING_TRY(hipStreamWaitEvent(s.inflate_stream, s.follower_carried, 0));
    ING_TRY(hipStreamWaitEvent(g->copy_stream, s.follower_carried, 0));
    s.has_follower = false;
  }
  return GMX_OK;
}

int gmx_ingest_submit_bgzf(gmx_ingest *g, int slot, const uint8_t *compressed, uint64_t n_bytes, const gmx_bgzf_member *members, uint64_t n_members,
                           int final_chunk) try {
  int rc = ing_begin(g, slot, "gmx_ingest_submit_bgzf");
  if (rc) return rc;
  if ((!compressed && n_bytes) || (!members && n_members) || n_bytes > g->max_comp || n_members > g->cap_members) {
    gmx_set_error("gmx_ingest_submit_bgzf: null argument, or more compressed bytes / members than the ingest was created for");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  uint64_t text = 0;
  for (uint64_t i = 0; i < n_members; ++i) {
    const gmx_bgzf_member &m = members[i];
    if (m.offset + m.size > n_bytes || m.isize > (1u << 16)) {
      gmx_set_error("gmx_ingest_submit_bgzf: member " + std::to_string(i) + " lies outside the bytes given, or holds more than 64 KB of text");
      return GMX_EINVAL;
    }
    s.h_members[i] = IngestMember{(uint32_t)m.offset, (uint32_t)m.size, (uint32_t)text, m.isize, m.crc32, 0u};
    text += m.isize;
  }
  if (text > g->max_text) {
    gmx_set_error("gmx_ingest_submit_bgzf: the members hold more text than the ingest was created for");
    return GMX_EINVAL;
  }
  // (the bit reader fetches up to 128 words ahead: the staging buffer has slack; the words right behind the data are zeroed)
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_comp, compressed, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipMemsetAsync(reinterpret_cast<uint8_t *>(s.d_comp) + n_bytes, 0, 16, g->copy_stream));
  if (n_members) ING_TRY(hipMemcpyAsync(s.d_members, s.h_members, n_members * sizeof(IngestMember), hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  return ing_enqueue_scan(g, slot, (uint32_t)text, final_chunk, true, (uint32_t)n_members);
} GMX_GUARD_INT("gmx_ingest_submit_bgzf")

int gmx_ingest_submit_text(gmx_ingest *g, int slot, const uint8_t *text, uint64_t n_bytes, int final_chunk) try {
  int rc = ing_begin(g, slot, "gmx_ingest_submit_text");
  if (rc) return rc;
  if ((!text && n_bytes) || n_bytes > g->max_text) {
    gmx_set_error("gmx_ingest_submit_text: null text, or more text than the ingest was created for");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_text + ING_CARRY_MAX, text, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  return ing_enqueue_scan(g, slot, (uint32_t)n_bytes, final_chunk, false, 0);
} GMX_GUARD_INT("gmx_ingest_submit_text")

// The buffers of the gzip route: at its first chunk, and again when a chunk has more pieces than they were made for (the old
// ones are freed: everything that used them ran on `stream`). Piece size GMX_GZ_PIECE (bytes; tests cut small files into many).
static int ing_gz_alloc(gmx_ingest *g, uint32_t n_pieces) {
  std::unique_ptr<gmx_ingest::Gz> z(new gmx_ingest::Gz());
  uint64_t piece = 32u << 10;
  if (const char *e = getenv("GMX_GZ_PIECE")) piece = std::min<uint64_t>(std::max<uint64_t>(64, (uint64_t)atoll(e)), 64u << 20);
  z->piece_bytes = (uint32_t)piece;
  z->max_pieces = std::max<uint32_t>(n_pieces, 4);
  // symbols a piece may write: its blocks and the one that reaches over its end (a zlib block holds up to 16 K symbols: 1 M symbols
  // is 64 bytes per symbol — FASTQ of one quality value inflates to less); beyond it GMX_INGEST_GZ_PIECE_BOUND
  z->cap = (uint32_t)((std::max<uint64_t>(piece * 32u, 1u << 20) + GZ_FLUSH - 1) / GZ_FLUSH * GZ_FLUSH);
  if (const char *e = getenv("GMX_GZ_TEST_FIND")) {  // test hook: "L,D" (gmx_gz_decode_kernel)
    z->late_mod = (uint32_t)atoi(e);
    if (const char *c = strchr(e, ',')) z->drop_mod = (uint32_t)atoi(c + 1);
  }
  g->allocs.reserve(g->allocs.size() + 8);
  if (g->gz) {  // (the window and the stream state go on)
    ING_TRY(hipStreamSynchronize(g->stream));
    for (void *p : {(void *)g->gz->d_pieces, (void *)g->gz->d_sym, (void *)g->gz->d_wins}) {
      g->allocs.erase(std::remove(g->allocs.begin(), g->allocs.end(), p), g->allocs.end());
      (void)hipFree(p);
    }
    z->d_window = g->gz->d_window;
    z->d_state = g->gz->d_state;
    delete g->gz;
    g->gz = nullptr;
  }
  int rc;
  if ((rc = ing_alloc(g, &z->d_pieces, z->max_pieces, true)) || (rc = ing_alloc(g, &z->d_sym, (size_t)z->max_pieces * z->cap + 64, false)) ||
      (rc = ing_alloc(g, &z->d_wins, (size_t)z->max_pieces * GZ_WIN, false)) || (!z->d_window && (rc = ing_alloc(g, &z->d_window, GZ_WIN, true))) ||
      (!z->d_state && (rc = ing_alloc(g, &z->d_state, 1, true))))
    return rc;
  g->gz = z.release();
  return GMX_OK;
}

int gmx_ingest_submit_gzip(gmx_ingest *g, int slot, const uint8_t *bytes, uint64_t n_bytes, uint64_t n_own, int final_chunk) try {
  if (g && g->format == GMX_INGEST_FORMAT_BAM) return ing_not_bam("gmx_ingest_submit_gzip");
  int rc = ing_begin(g, slot, "gmx_ingest_submit_gzip");
  if (rc) return rc;
  if ((!bytes && n_bytes) || n_own > n_bytes || n_bytes > g->max_comp || n_bytes >= (1u << 29) || (final_chunk && n_bytes != n_own)) {
    gmx_set_error("gmx_ingest_submit_gzip: null bytes, n_own > n_bytes, look-ahead given with the final chunk, or more bytes than "
                  "gmx_ingest_max_compressed() / 512 MB");
    return GMX_EINVAL;
  }
  {
    uint64_t piece = 32u << 10;  // (as ing_gz_alloc)
    if (g->gz) piece = g->gz->piece_bytes;
    else if (const char *e = getenv("GMX_GZ_PIECE")) piece = std::min<uint64_t>(std::max<uint64_t>(64, (uint64_t)atoll(e)), 64u << 20);
    const uint32_t need = (uint32_t)std::max<uint64_t>(1, (n_own + piece - 1) / piece);
    if ((!g->gz || g->gz->max_pieces < need) && (rc = ing_gz_alloc(g, need))) return rc;
  }
  gmx_ingest::Gz &z = *g->gz;
  gmx_ingest::Slot &s = g->slot[slot];
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_comp, bytes, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipMemsetAsync(reinterpret_cast<uint8_t *>(s.d_comp) + n_bytes, 0, 16, g->copy_stream));  // (the bit reader's words behind the bytes)
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  ING_TRY(hipStreamWaitEvent(g->stream, s.copied, 0));
  GzArgs a;
  a.comp = s.d_comp;
  a.n_bytes = (uint32_t)n_bytes;
  a.n_own = (uint32_t)n_own;
  a.final_chunk = final_chunk ? 1u : 0u;
  a.fresh = g->gz_fresh ? 1u : 0u;
  a.piece_bits = z.piece_bytes * 8u;
  a.n_pieces = (uint32_t)std::max<uint64_t>(1, (n_own + z.piece_bytes - 1) / z.piece_bytes);
  a.cap = z.cap;
  a.sym = z.d_sym;
  a.pieces = z.d_pieces;
  a.st = z.d_state;
  a.debug = getenv("GMX_GZ_DEBUG") ? 1u : 0u;
  a.late_mod = z.late_mod;
  a.drop_mod = z.drop_mod;
  uint8_t *const text = s.d_text + ING_CARRY_MAX;
  hipLaunchKernelGGL(gmx_gz_decode_kernel, dim3(a.n_pieces), dim3(64), 0, g->stream, a);
  hipLaunchKernelGGL(gmx_gz_link_kernel, dim3(1), dim3(64), 0, g->stream, a, (uint64_t)g->max_text);
  hipLaunchKernelGGL(gmx_gz_window_kernel, dim3(1), dim3(1024), 0, g->stream, a, z.d_wins, z.d_window);
  hipLaunchKernelGGL(gmx_gz_resolve_kernel, dim3(a.n_pieces, 16), dim3(256), 0, g->stream, a, (const uint8_t *)z.d_wins, text);
  hipLaunchKernelGGL(gmx_gz_crc_kernel, dim3(a.n_pieces), dim3(64), 0, g->stream, a, (const uint8_t *)text);
  hipLaunchKernelGGL(gmx_gz_check_kernel, dim3(1), dim3(64), 0, g->stream, a, s.d_inflate_status);
  ING_TRY(hipGetLastError());
  g->gz_fresh = false;
  return ing_enqueue_scan(g, slot, 0, final_chunk, false, 0, 0xFFFFFFFFu, &z.d_state->text_len);
} GMX_GUARD_INT("gmx_ingest_submit_gzip")

int64_t gmx_ingest_gzip_repairs(gmx_ingest *g) try {
  if (!g) {
    gmx_set_error("null ingest");
    return GMX_EINVAL;
  }
  if (!g->gz) return 0;
  ING_TRY(hipSetDevice(g->device));
  ING_TRY(hipStreamSynchronize(g->stream));
  uint32_t v = 0;
  ING_TRY(hipMemcpy(&v, &g->gz->d_state->repairs, 4, hipMemcpyDeviceToHost));
  return (int64_t)v;
} GMX_GUARD_INT("gmx_ingest_gzip_repairs")

// Chunks dealt over several devices (one ingest per device): the cut record at a chunk's start lies on ANOTHER device, so a chunk
// is uploaded and inflated at once (_deferred) and scanned (gmx_ingest_scan) when the caller has the end of the chunk before —
// gmx_ingest_fetch_tail of that chunk's slot, on its device — which it hands over as host bytes.
int gmx_ingest_submit_bgzf_deferred(gmx_ingest *g, int slot, const uint8_t *compressed, uint64_t n_bytes, const gmx_bgzf_member *members, uint64_t n_members) try {
  if (g && g->format == GMX_INGEST_FORMAT_BAM) return ing_not_bam("gmx_ingest_submit_bgzf_deferred");
  if (g) g->last_slot = -1;  // (nothing is carried on the device in this mode: the slots need not alternate)
  int rc = ing_begin(g, slot, "gmx_ingest_submit_bgzf_deferred");
  if (rc) return rc;
  if ((!compressed && n_bytes) || (!members && n_members) || n_bytes > g->max_comp || n_members > g->cap_members) {
    gmx_set_error("gmx_ingest_submit_bgzf_deferred: null argument, or more compressed bytes / members than the ingest was created for");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  uint64_t text = 0;
  for (uint64_t i = 0; i < n_members; ++i) {
    const gmx_bgzf_member &m = members[i];
    if (m.offset + m.size > n_bytes || m.isize > (1u << 16)) {
      gmx_set_error("gmx_ingest_submit_bgzf_deferred: member " + std::to_string(i) + " lies outside the bytes given, or holds more than 64 KB of text");
      return GMX_EINVAL;
    }
    s.h_members[i] = IngestMember{(uint32_t)m.offset, (uint32_t)m.size, (uint32_t)text, m.isize, m.crc32, 0u};
    text += m.isize;
  }
  if (text > g->max_text) {
    gmx_set_error("gmx_ingest_submit_bgzf_deferred: the members hold more text than the ingest was created for");
    return GMX_EINVAL;
  }
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_comp, compressed, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipMemsetAsync(reinterpret_cast<uint8_t *>(s.d_comp) + n_bytes, 0, 16, g->copy_stream));
  if (n_members) ING_TRY(hipMemcpyAsync(s.d_members, s.h_members, n_members * sizeof(IngestMember), hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  rc = ing_enqueue_inflate(g, slot, (uint32_t)n_members);
  if (rc) return rc;
  s.deferred = true;
  s.deferred_inflate = true;
  s.deferred_text = (uint32_t)text;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_submit_bgzf_deferred")

// The same for a chunk of plain text (an uncompressed FASTQ dealt over several devices): uploaded at once, scanned by gmx_ingest_scan.
int gmx_ingest_submit_text_deferred(gmx_ingest *g, int slot, const uint8_t *text, uint64_t n_bytes) try {
  if (g && g->format == GMX_INGEST_FORMAT_BAM) return ing_not_bam("gmx_ingest_submit_text_deferred");
  if (g) g->last_slot = -1;
  int rc = ing_begin(g, slot, "gmx_ingest_submit_text_deferred");
  if (rc) return rc;
  if ((!text && n_bytes) || n_bytes > g->max_text) {
    gmx_set_error("gmx_ingest_submit_text_deferred: null text, or more text than the ingest was created for");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_text + ING_CARRY_MAX, text, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  s.deferred = true;
  s.deferred_inflate = false;
  s.deferred_text = (uint32_t)n_bytes;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_submit_text_deferred")

int gmx_ingest_scan(gmx_ingest *g, int slot, const uint8_t *carry, uint64_t n_carry, int final_chunk) try {
  if (g && g->format == GMX_INGEST_FORMAT_BAM) return ing_not_bam("gmx_ingest_scan");
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || !g->slot[slot].deferred || (!carry && n_carry) || n_carry > ING_CARRY_MAX) {
    gmx_set_error("gmx_ingest_scan: null ingest, slot without a gmx_ingest_submit_bgzf_deferred chunk, or more than 1 MB of carried text (a record that long is not FASTQ)");
    return GMX_EINVAL;
  }
  ING_TRY(hipSetDevice(g->device));
  gmx_ingest::Slot &s = g->slot[slot];
  // the carried bytes right in front of the members' text (pageable memory: the copy is over when the call returns)
  if (n_carry) ING_TRY(hipMemcpyAsync(s.d_text + ING_CARRY_MAX - n_carry, carry, n_carry, hipMemcpyHostToDevice, g->stream));
  return ing_enqueue_scan(g, slot, s.deferred_text, final_chunk, s.deferred_inflate, 0, (uint32_t)n_carry);
} GMX_GUARD_INT("gmx_ingest_scan")

int64_t gmx_ingest_fetch_tail(gmx_ingest *g, int slot, uint8_t *out, uint64_t cap) try {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || g->slot[slot].in_flight) {
    gmx_set_error("gmx_ingest_fetch_tail: null ingest, bad slot, or the slot's chunk is still in flight");
    return GMX_EINVAL;
  }
  const IngestState &st = *g->slot[slot].h_state;
  if (!out) return (int64_t)st.tail_len;
  if (cap < st.tail_len) {
    gmx_set_error("gmx_ingest_fetch_tail: buffer too small");
    return GMX_EINVAL;
  }
  if (st.tail_len && (hipSetDevice(g->device) != hipSuccess ||
                      hipMemcpy(out, g->slot[slot].d_text + st.consumed, st.tail_len, hipMemcpyDeviceToHost) != hipSuccess)) {
    gmx_set_error("gmx_ingest_fetch_tail: hipMemcpy failed");
    return GMX_EHIP;
  }
  return (int64_t)st.tail_len;
} GMX_GUARD_INT("gmx_ingest_fetch_tail")

int gmx_ingest_wait(gmx_ingest *g, int slot, gmx_ingest_result *out) try {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || !out) {
    gmx_set_error("gmx_ingest_wait: null argument or slot not 0 / 1 / 2");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  if (!s.in_flight) {
    gmx_set_error("gmx_ingest_wait: nothing was submitted to the slot");
    return GMX_EINVAL;
  }
  ING_TRY(hipSetDevice(g->device));
  ING_TRY(hipEventSynchronize(s.done));
  s.in_flight = false;
  const IngestState &st = *s.h_state;
  memset(out, 0, sizeof(*out));
  out->status = st.flags;
  out->bad_member = st.bad_member;
  out->n_reads = st.n_reads;
  out->n_bases = st.n_bases;
  out->uniform_len = st.uniform_len;
  out->any_skip = st.any_skip;
  out->n_pairs = st.n_pairs;
  out->text_bytes = st.text_len;
  out->consumed_bytes = st.consumed - st.text_start;
  out->tail_bytes = st.tail_len;
  for (int i = 0; i < 16; ++i) out->sub_pairs[i] = st.sub_pairs[i];
  out->d_planes = reinterpret_cast<const uint64_t *>(s.d_planes);
  out->d_offsets = st.uniform_len ? nullptr : reinterpret_cast<const uint64_t *>(s.d_offsets);
  out->d_skip = s.d_skip;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_wait")

int gmx_ingest_release_after(gmx_ingest *g, int slot, void *hip_stream) try {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS) {
    gmx_set_error("gmx_ingest_release_after: null ingest or slot not 0 / 1 / 2");
    return GMX_EINVAL;
  }
  ING_TRY(hipSetDevice(g->device));
  gmx_ingest::Slot &s = g->slot[slot];
  if (s.has_release) {  // a second stream behind the same chunk
    ING_TRY(hipEventRecord(s.released2, (hipStream_t)hip_stream));
    s.has_release2 = true;
  } else {
    ING_TRY(hipEventRecord(s.released, (hipStream_t)hip_stream));
    s.has_release = true;
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_release_after")

int64_t gmx_ingest_fetch_text(gmx_ingest *g, int slot, uint8_t *out, uint64_t cap) try {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || g->slot[slot].in_flight) {
    gmx_set_error("gmx_ingest_fetch_text: null ingest, bad slot, or the slot's chunk is still in flight");
    return GMX_EINVAL;
  }
  const IngestState &st = *g->slot[slot].h_state;
  if (!out) return (int64_t)st.text_len;
  if (cap < st.text_len) {
    gmx_set_error("gmx_ingest_fetch_text: buffer too small");
    return GMX_EINVAL;
  }
  if (hipSetDevice(g->device) != hipSuccess || hipMemcpy(out, g->slot[slot].d_text + st.text_start, st.text_len, hipMemcpyDeviceToHost) != hipSuccess) {
    gmx_set_error("gmx_ingest_fetch_text: hipMemcpy failed");
    return GMX_EHIP;
  }
  return (int64_t)st.text_len;
} GMX_GUARD_INT("gmx_ingest_fetch_text")

int gmx_ingest_fetch_reads(gmx_ingest *g, int slot, uint64_t *planes, uint64_t *offsets, uint8_t *skip) try {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || g->slot[slot].in_flight) {
    gmx_set_error("gmx_ingest_fetch_reads: null ingest, bad slot, or the slot's chunk is still in flight");
    return GMX_EINVAL;
  }
  const gmx_ingest::Slot &s = g->slot[slot];
  const IngestState &st = *s.h_state;
  ING_TRY(hipSetDevice(g->device));
  if (planes && st.n_pairs) ING_TRY(hipMemcpy(planes, s.d_planes, st.n_pairs * 8, hipMemcpyDeviceToHost));
  if (offsets && !st.uniform_len && st.n_reads) ING_TRY(hipMemcpy(offsets, s.d_offsets, ((size_t)st.n_reads + 1) * 8, hipMemcpyDeviceToHost));
  if (skip && st.n_reads) ING_TRY(hipMemcpy(skip, s.d_skip, st.n_reads, hipMemcpyDeviceToHost));
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_fetch_reads")

}  // extern "C"

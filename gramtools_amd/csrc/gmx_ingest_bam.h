// gmx_ingest_bam.h — part of gmx_ingest.hip: BAM records chained, linked and packed.
#pragma once

namespace {

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
// (The loop around the arithmetic is ing_pack_words' own, written out: inside that frame this kernel measured 2 % slower, 48.5 us a
// chunk against 47.4, outside the spread of its runs — profiles/ingest_refactor. A change to the frame is made here too.)
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

}  // namespace

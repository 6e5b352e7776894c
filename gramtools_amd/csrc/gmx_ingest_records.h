// gmx_ingest_records.h — part of gmx_ingest.hip: a chunk's text -> records -> bit planes (FASTQ, FASTA, LINES) and the pack frame.
#pragma once

namespace {

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
// TRIM (gmx_ingest_set_quality_trim): the lane runs gmx_qtrim_length over its record's quality line, and the
// trimmed length t takes the read's place in everything downstream: rec_len, the min / max / sum reduction (hence uniform_len,
// the offsets, the planes). t < min_length sets the read's skip flag here (the pack kernel adds the letters' verdict on [0, t)).
// The malformed-record test stays on the lengths as they lie in the text. trim[4]: reads shortened, bases removed, reads
// skipped for t < min_length, bases before trimming. Two kernels around this one body, so that an ingest without trimming
// launches the code object it always did (gmx_records_kernel: no argument, no branch added).
template <bool TRIM>
__device__ __forceinline__ void ing_records(const uint8_t *text, IngestState *st, const uint32_t *line_end, uint32_t *rec_start, uint32_t *rec_len, uint8_t *skip,
                                            uint32_t cap_reads, uint32_t first, uint32_t stride, uint32_t min_quality, uint32_t min_length, unsigned long long *trim) {
  // (first, stride: the grid-stride loop's, worked out by the kernels themselves — the block and grid sizes are folded into loads of
  //  the dispatch packet only where a kernel's own text asks for them, and gmx_records_kernel is to stay the code it was)
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
  [[maybe_unused]] unsigned long long bases_in = 0, removed = 0;
  [[maybe_unused]] uint32_t shortened = 0, too_short = 0;
  [[maybe_unused]] bool any_short = false;
  for (uint32_t r = first; r < n_reads; r += stride) {
    const uint32_t s1 = r ? line_end[4u * r - 1u] + 1u : lo;
    const uint32_t e1 = le(4u * r), e2 = le(4u * r + 1u), e3 = le(4u * r + 2u), e4 = le(4u * r + 3u);
    const uint32_t s2 = e1 + 1u, s3 = e2 + 1u, s4 = e3 + 1u;
    uint32_t n = e2 - s2, nq = e4 >= s4 ? e4 - s4 : 0u;
    if (n && text[s2 + n - 1u] == '\r') --n;
    if (nq && text[s4 + nq - 1u] == '\r') --nq;
    if (text[s1] != '@' || s3 >= hi || text[s3] != '+' || nq != n || n == 0) bad = true;
    rec_start[r] = s2;
    if constexpr (TRIM) {
      if (nq == n && n) {  // (a malformed record is reported below: its reads are never used)
        const uint32_t t = gmx_qtrim_length(text + s4, n, min_quality);
        bases_in += n;
        if (t < n) {
          ++shortened;
          removed += n - t;
        }
        if (t < min_length) {
          ++too_short;
          any_short = true;
        }
        n = t;
      }
    }
    rec_len[r] = n;
    skip[r] = TRIM && n < min_length ? 1 : 0;
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
      // fewer than four lines at the end of the file (more records than there is room for are well-formed: TOO_MANY_LINES alone)
      if (st->final_chunk && hi != lo && !too_many) atomicOr(&st->flags, GMX_INGEST_BAD_RECORD);
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
  if constexpr (TRIM) {
    for (int off = 32; off > 0; off >>= 1) {
      shortened += __shfl_down(shortened, off);
      too_short += __shfl_down(too_short, off);
      removed += __shfl_down(removed, off);
      bases_in += __shfl_down(bases_in, off);
    }
    const unsigned long long some_short = __ballot(any_short);
    if ((threadIdx.x & 63u) == 0) {
      if (shortened) atomicAdd(&trim[0], (unsigned long long)shortened);
      if (removed) atomicAdd(&trim[1], removed);
      if (too_short) atomicAdd(&trim[2], (unsigned long long)too_short);
      if (bases_in) atomicAdd(&trim[3], bases_in);
      if (some_short) st->any_skip = 1;
    }
  }
}
__global__ void __launch_bounds__(256) gmx_records_kernel(const uint8_t *text, IngestState *st, const uint32_t *line_end, uint32_t *rec_start,
                                                          uint32_t *rec_len, uint8_t *skip, uint32_t cap_reads) {
  ing_records<false>(text, st, line_end, rec_start, rec_len, skip, cap_reads, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, 0u, 0u, nullptr);
}
__global__ void __launch_bounds__(256) gmx_records_trim_kernel(const uint8_t *text, IngestState *st, const uint32_t *line_end, uint32_t *rec_start,
                                                               uint32_t *rec_len, uint8_t *skip, uint32_t cap_reads, uint32_t min_quality, uint32_t min_length,
                                                               unsigned long long *trim) {
  ing_records<true>(text, st, line_end, rec_start, rec_len, skip, cap_reads, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, min_quality, min_length, trim);
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
// (bit 2 of the ASCII code is the code's high bit, bit 1 XOR bit 2 the low one: 'A' 0x41 'C' 0x43 'G' 0x47 'T' 0x54, either case).
// ing_pack_letters: letters src[0, m) -> bits [at, at + m) of a pair of planes
__device__ __forceinline__ void ing_pack_letters(const uint8_t *src, uint32_t m, uint32_t at, uint32_t &lo, uint32_t &hi, bool &ok) {
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t c = src[j], u = c & 0xDFu;
    ok = ok && (u == 0x41u || u == 0x43u || u == 0x47u || u == 0x54u);
    const uint32_t h = (c >> 2) & 1u;
    hi |= h << (at + j);
    lo |= (((c >> 1) & 1u) ^ h) << (at + j);
  }
}
// The frame of the pack kernels (gmx_fq_pack_kernel, gmx_seq_pack_kernel; gmx_bam_pack_kernel has the same loop written out, see
// there): grid-stride over (read r, word w) of the chunk, the word's place in the planes in the uniform and in the offsets form
// (include/gmx.h), the store, the skip flag. src(r, w, len, m, lo, hi, ok) turns bases [32 w, 32 w + m) of read r, 1 <= m <= 32,
// into a pair of planes.
template <class Src>
__device__ __forceinline__ void ing_pack_words(IngestState *st, const uint32_t *rec_len, const unsigned long long *offsets, unsigned long long *planes, uint8_t *skip,
                                               Src src) {
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
    if (w * 32u < len) src(r, w, len, min(32u, len - w * 32u), lo, hi, ok);
    planes[first + w] = (unsigned long long)lo | ((unsigned long long)hi << 32);
    if (!ok) {
      skip[r] = 1;
      st->any_skip = 1;
    }
  }
}
__global__ void __launch_bounds__(256) gmx_fq_pack_kernel(const uint8_t *text, IngestState *st, const uint32_t *rec_start, const uint32_t *rec_len,
                                                          const unsigned long long *offsets, unsigned long long *planes, uint8_t *skip) {
  ing_pack_words(st, rec_len, offsets, planes, skip, [=](uint32_t r, uint32_t w, uint32_t, uint32_t m, uint32_t &lo, uint32_t &hi, bool &ok) {
    ing_pack_letters(text + rec_start[r] + w * 32u, m, 0u, lo, hi, ok);
  });
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
__global__ void __launch_bounds__(256) gmx_seq_pack_kernel(const uint8_t *text, IngestState *st, const uint32_t *line_end, const uint32_t *line_base,
                                                           const uint32_t *rec_line, const uint32_t *rec_start, const uint32_t *rec_len,
                                                           const unsigned long long *offsets, unsigned long long *planes, uint8_t *skip) {
  const uint32_t text_lo = st->text_start;
  ing_pack_words(st, rec_len, offsets, planes, skip, [=](uint32_t r, uint32_t w, uint32_t, uint32_t m, uint32_t &lo, uint32_t &hi, bool &ok) {
    const uint32_t start = rec_start[r];
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
  });
}

}  // namespace

// gmx_qtrim.h — quality trimming of a read's 3' end: the running-sum rule of BWA (`bwa aln -q`) and cutadapt (`-q`), Phred+33.
// One text for the device's record scan (gmx_ingest_records.h) and for `gram`'s host reader (gram_main.cpp); DESIGN.md §11.5.
//
//   q_i = max(byte_i - 33, 0);  s = 0, best = 0, t = n;  for i = n - 1 down to 0: s += Q - q_i; s < 0: stop; s > best: best = s, t = i
//
// The read keeps bases [0, t). A good last base ends the loop at once; a tie keeps the longer read; a read that is poor
// throughout ends with t = 0.
#pragma once
#include <stdint.h>

#ifndef GMX_HD
#if defined(__HIPCC__)
#define GMX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GMX_HD inline
#endif
#endif

#define GMX_QTRIM_MAX_QUALITY 93u  // Phred+33 ends at '~'

// Device code fetches the line in ALIGNED 32-bit words from its end backwards — one load serves four steps, and the one word most
// lanes ever need is a single dword load; neighbouring lanes' lines lie a record apart, so nothing coalesces either way. The word
// that holds the line's first (last) byte reaches up to three bytes below (beyond) it: the ingest's text buffer has the room, and
// the bytes are never looked at. Host code reads byte by byte: its strings have no such room.
GMX_HD uint32_t gmx_qtrim_length(const uint8_t *qual, uint32_t n, uint32_t min_quality) {
  long long s = 0, best = 0;  // (a record may hold 2^31 bases: 93 a base does not fit 32 bits)
  uint32_t t = n;
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t word = 0;
#endif
  for (uint32_t i = n; i-- > 0;) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t in_word = (uint32_t)(reinterpret_cast<uintptr_t>(qual + i) & 3u);
    if (i == n - 1u || in_word == 3u) word = *reinterpret_cast<const uint32_t *>(qual + i - in_word);
    const uint32_t byte = (word >> (8u * in_word)) & 0xFFu;
#else
    const uint32_t byte = qual[i];
#endif
    s += (long long)min_quality - (long long)(byte > 33u ? byte - 33u : 0u);
    if (s < 0) break;
    if (s > best) {
      best = s;
      t = i;
    }
  }
  return t;
}

// gmx_ingest_state.h — part of gmx_ingest.hip: the error macro, the device-side state of a chunk, the member table.
#pragma once

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

}  // namespace

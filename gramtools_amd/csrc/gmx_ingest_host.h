// gmx_ingest_host.h — part of gmx_ingest.hip: the ingest object, the launches of a chunk, the C ABI.
#pragma once

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
    unsigned long long *d_trim = nullptr, *h_trim = nullptr;  // gmx_ingest_set_quality_trim: the chunk's four counters (gmx_ingest_trim_stats)
    IngestMember *h_members = nullptr;  // page-locked staging of the member table
    IngestInflateStatus *d_inflate_status = nullptr;
    hipStream_t inflate_stream = nullptr;  // the slot's inflate kernel: beside the scan of the chunk before and the tail of its inflate kernel
    hipEvent_t copied = nullptr, done = nullptr, inflated = nullptr, carried = nullptr;
    hipEvent_t released[2] = {nullptr, nullptr};  // gmx_ingest_release_after: the first n_release of them are recorded (an engine with
    int n_release = 0;                            // two workspaces records a second one, behind the launches on its second stream)
    bool in_flight = false, has_carried = false;
    hipEvent_t follower_carried = nullptr;  // `carried` of the chunk that continued this slot's: its carry kernel read the end of this slot's text
    bool has_follower = false;
    bool deferred = false;       // gmx_ingest_submit_bgzf_deferred / _text_deferred: uploaded (and inflating), scan still to come (gmx_ingest_scan)
    bool deferred_inflate = true;  // ... with an inflate kernel (false: the chunk arrived as text)
    uint32_t deferred_text = 0;  // ... bytes of text of its members
  } slot[GMX_INGEST_SLOTS];
  int last_slot = -1;  // the slot whose chunk the next one continues (-1: a file's first chunk)
  int format = GMX_INGEST_FORMAT_FASTQ;  // gmx_ingest_set_format
  uint32_t trim_quality = 0, trim_min_length = 0;  // gmx_ingest_set_quality_trim (0: off)
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
template <class T>
int ing_alloc_once(gmx_ingest *g, T **p, size_t count) {
  return *p ? GMX_OK : ing_alloc(g, p, count, false);
}
// The optional tables of a format (gmx_ingest_set_format), `per_slot` of them in every slot: tables(slot) allocates those the
// slot does not have yet (the caller asks when the LAST slot lacks one: a call that failed half-way goes on where it stopped)
template <class F>
int ing_slot_tables(gmx_ingest *g, size_t per_slot, F tables) {
  ING_TRY(hipSetDevice(g->device));
  g->allocs.reserve(g->allocs.size() + per_slot * GMX_INGEST_SLOTS + 1);
  for (auto &s : g->slot)
    if (int rc = tables(s)) return rc;
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
        (rc = ing_alloc(g, &s.d_state, 1, true)) || (rc = ing_alloc(g, &s.d_inflate_status, 1, true)) || (rc = ing_alloc(g, &s.d_trim, 4, true)))
      return fail(rc);
    if (hipHostMalloc(reinterpret_cast<void **>(&s.h_state), sizeof(IngestState), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&s.h_trim), 4 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&s.h_members), (size_t)g->cap_members * sizeof(IngestMember), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&s.copied, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.done, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess ||
        hipEventCreateWithFlags(&s.released[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&s.released[1], hipEventDisableTiming) != hipSuccess ||
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
    if (s.h_trim) (void)hipHostFree(s.h_trim);
    if (s.h_members) (void)hipHostFree(s.h_members);
    if (s.copied) (void)hipEventDestroy(s.copied);
    if (s.done) (void)hipEventDestroy(s.done);
    for (hipEvent_t e : s.released)
      if (e) (void)hipEventDestroy(e);
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
  if (format == GMX_INGEST_FORMAT_BAM && g->trim_quality) {
    gmx_set_error("gmx_ingest_set_format: BAM records are not trimmed on the device (gmx_ingest_set_quality_trim is on: switch it off, or read the file on the host)");
    return GMX_EINVAL;
  }
  int rc;
  if (format == GMX_INGEST_FORMAT_BAM && !g->slot[GMX_INGEST_SLOTS - 1].d_bam_rev) {  // the tile tables, once
    uint64_t tile = 4096;
    if (const char *e = getenv("GMX_BAM_TILE")) tile = std::min<uint64_t>(std::max<uint64_t>(64, (uint64_t)atoll(e)), 1u << 20);
    g->bam_tile = (uint32_t)tile;
    g->bam_tiles_max = (uint32_t)((g->max_text + tile - 1) / tile + 1);
    g->bam_room = (uint32_t)(tile / BAM_REC_MIN + 3);  // (records of >= 37 bytes that start in a tile, and the carried one in front of tile 0)
    const size_t n = g->bam_tiles_max;
    rc = ing_slot_tables(g, 7, [&](gmx_ingest::Slot &s) {
      int rc;
      if ((rc = ing_alloc_once(g, &s.d_bam_guess, n)) || (rc = ing_alloc_once(g, &s.d_bam_exit, n)) || (rc = ing_alloc_once(g, &s.d_bam_count, n)) ||
          (rc = ing_alloc_once(g, &s.d_bam_flag, n)) || (rc = ing_alloc_once(g, &s.d_bam_starts, n * g->bam_room)) ||
          (rc = ing_alloc_once(g, &s.d_bam_blk, n / ING_SCAN_BLOCK + 2)) || (rc = ing_alloc_once(g, &s.d_bam_rev, g->cap_reads)))
        return rc;
      // (the counter last: the tables are asked for again as long as the last slot's d_bam_rev is missing)
      return g->d_bam_rewalks ? GMX_OK : ing_alloc(g, &g->d_bam_rewalks, 1, true);
    });
    if (rc) return rc;
  }
  if (format != GMX_INGEST_FORMAT_FASTQ && format != GMX_INGEST_FORMAT_BAM && !g->slot[GMX_INGEST_SLOTS - 1].d_line_blk) {  // the line tables, once
    rc = ing_slot_tables(g, 4, [&](gmx_ingest::Slot &s) {
      int rc;
      if ((rc = ing_alloc_once(g, &s.d_line_rec, (size_t)g->cap_lines + 2)) || (rc = ing_alloc_once(g, &s.d_line_base, (size_t)g->cap_lines + 2)) ||
          (rc = ing_alloc_once(g, &s.d_rec_line, (size_t)g->cap_reads + 2)) || (rc = ing_alloc_once(g, &s.d_line_blk, (size_t)g->cap_lines / ING_SCAN_BLOCK + 2)))
        return rc;
      return GMX_OK;
    });
    if (rc) return rc;
  }
  g->format = format;
  g->bam_header_left = 0;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_set_format")

int gmx_ingest_set_quality_trim(gmx_ingest *g, uint32_t min_quality, uint32_t min_length) try {
  if (!g || min_quality > GMX_QTRIM_MAX_QUALITY || (min_quality && min_length < 1)) {
    gmx_set_error("gmx_ingest_set_quality_trim: null ingest, min_quality above 93, or min_length 0 (min_quality 0 switches trimming off)");
    return GMX_EINVAL;
  }
  for (const auto &s : g->slot)
    if (s.in_flight || s.deferred) {
      gmx_set_error("gmx_ingest_set_quality_trim: a slot's chunk is in flight (trimming is set between files)");
      return GMX_EINVAL;
    }
  if (min_quality && g->format == GMX_INGEST_FORMAT_BAM) {
    gmx_set_error("gmx_ingest_set_quality_trim: BAM records are not trimmed on the device (read the file on the host)");
    return GMX_EINVAL;
  }
  g->trim_quality = min_quality;
  g->trim_min_length = min_quality ? min_length : 0;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_set_quality_trim")

int gmx_ingest_trim_stats(gmx_ingest *g, int slot, uint64_t out[4]) try {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || !out || g->slot[slot].in_flight || g->slot[slot].deferred) {
    gmx_set_error("gmx_ingest_trim_stats: null argument, bad slot, or the slot's chunk is still in flight (after its gmx_ingest_wait)");
    return GMX_EINVAL;
  }
  for (int i = 0; i < 4; ++i) out[i] = g->slot[slot].h_trim[i];
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_trim_stats")

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

// a counter the kernels on `stream` add to (null: its route has not run yet), after everything enqueued there
static int64_t ing_read_counter(gmx_ingest *g, const uint32_t *d_counter) {
  if (!g) {
    gmx_set_error("null ingest");
    return GMX_EINVAL;
  }
  if (!d_counter) return 0;
  ING_TRY(hipSetDevice(g->device));
  ING_TRY(hipStreamSynchronize(g->stream));
  uint32_t v = 0;
  ING_TRY(hipMemcpy(&v, d_counter, 4, hipMemcpyDeviceToHost));
  return (int64_t)v;
}

int64_t gmx_ingest_bam_rewalks(gmx_ingest *g) try {
  return ing_read_counter(g, g ? g->d_bam_rewalks : nullptr);
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
// What a chunk is, for ing_enqueue_scan: where its text comes from and what is carried in front of it.
struct IngChunk {
  uint32_t text_len = 0;                  // bytes of text of its members, known to the host ...
  const uint32_t *d_text_len = nullptr;   // ... or held by the device (plain gzip: the newline kernels get a grid for max_text, the tiles
                                          // beyond the text leave at once)
  bool inflate_now = false;               // the slot's inflate kernel is enqueued here, for n_members members
  uint32_t n_members = 0;
  bool inflate_status = false;            // the text was decoded on the device: the decoder's status word goes into the chunk's state
  bool carry_on_device = true;            // the cut record comes from the chunk before on this device (g->last_slot) ...
  uint32_t host_carry = 0;                // ... or the caller has put that many bytes in front of the text
  int final_chunk = 0;
};

// The end of every chunk's chain, behind the kernels that found its records: layout, offsets, the format's pack kernel, the state's way home.
static int ing_enqueue_tail(gmx_ingest *g, int si, const IngChunk &c) {
  gmx_ingest::Slot &s = g->slot[si];
  const uint32_t n_off_blk = (uint32_t)((g->cap_reads + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK);  // (the chunk's read count is on the device: blocks beyond it leave at once)
  hipLaunchKernelGGL(gmx_layout_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, c.inflate_status ? s.d_inflate_status : nullptr);
  hipLaunchKernelGGL(gmx_offsets1_kernel, dim3(n_off_blk), dim3(64), 0, g->stream, s.d_state, s.d_rec_len, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_offsets2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, s.d_offsets, s.d_off_blk);
  hipLaunchKernelGGL(gmx_offsets3_kernel, dim3(n_off_blk), dim3(64), 0, g->stream, s.d_state, s.d_offsets, s.d_off_blk);
  if (g->format == GMX_INGEST_FORMAT_FASTQ)
    hipLaunchKernelGGL(gmx_fq_pack_kernel, dim3(4096), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_rec_start, s.d_rec_len, s.d_offsets, s.d_planes, s.d_skip);
  else if (g->format == GMX_INGEST_FORMAT_BAM)
    hipLaunchKernelGGL(gmx_bam_pack_kernel, dim3(4096), dim3(256), 0, g->stream, (const uint8_t *)s.d_text, s.d_state, (const uint32_t *)s.d_rec_start,
                       (const uint32_t *)s.d_rec_len, (const uint8_t *)s.d_bam_rev, (const unsigned long long *)s.d_offsets, s.d_planes, s.d_skip);
  else
    hipLaunchKernelGGL(gmx_seq_pack_kernel, dim3(4096), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_line_end, s.d_line_base, s.d_rec_line, s.d_rec_start,
                       s.d_rec_len, s.d_offsets, s.d_planes, s.d_skip);
  ING_TRY(hipGetLastError());
  ING_TRY(hipMemcpyAsync(s.h_state, s.d_state, sizeof(IngestState), hipMemcpyDeviceToHost, g->stream));
  if (g->trim_quality && g->format == GMX_INGEST_FORMAT_FASTQ)  // (the only format with qualities to trim by: the others' counters stay zero)
    ING_TRY(hipMemcpyAsync(s.h_trim, s.d_trim, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, g->stream));
  else
    memset(s.h_trim, 0, 4 * sizeof(unsigned long long));  // (nothing of the slot is in flight: ing_begin)
  ING_TRY(hipEventRecord(s.done, g->stream));
  s.in_flight = true;
  s.deferred = false;
  g->last_slot = c.carry_on_device ? si : -1;  // (a chunk scanned with a host-provided start carries nothing on the device)
  return GMX_OK;
}

// BAM: the record chain behind the carry kernel (ing_enqueue_scan; chunks with the cut record on the device only)
static void ing_enqueue_bam(gmx_ingest *g, int si, uint32_t members_text) {
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
}

static int ing_enqueue_scan(gmx_ingest *g, int si, const IngChunk &c) {
  gmx_ingest::Slot &s = g->slot[si];
  gmx_ingest::Slot *prev = c.carry_on_device && g->last_slot >= 0 ? &g->slot[g->last_slot] : nullptr;
  if (c.inflate_now) {
    int rc = ing_enqueue_inflate(g, si, c.n_members);
    if (rc) return rc;
  }
  const uint32_t final_chunk = c.final_chunk ? 1 : 0;
  if (c.d_text_len)
    hipLaunchKernelGGL(gmx_carry_gz_kernel, dim3(64), dim3(256), 0, g->stream, prev ? prev->d_state : nullptr, prev ? prev->d_text : nullptr, s.d_state, s.d_text,
                       c.d_text_len, final_chunk);
  else
    hipLaunchKernelGGL(gmx_carry_kernel, dim3(64), dim3(256), 0, g->stream, prev ? prev->d_state : nullptr, prev ? prev->d_text : nullptr, s.d_state, s.d_text,
                       c.text_len, final_chunk, c.carry_on_device ? 0u : c.host_carry);
  ING_TRY(hipEventRecord(s.carried, g->stream));
  s.has_carried = true;
  if (prev) {  // (the slot of the chunk before may be overwritten once this kernel has read its end: ing_begin)
    prev->follower_carried = s.carried;
    prev->has_follower = true;
  }
  // (the gzip decoder ran on `stream` itself; the slot's inflate kernel, enqueued here or by a _deferred call, on a stream of its own)
  ING_TRY(hipStreamWaitEvent(g->stream, c.inflate_status && !c.d_text_len ? s.inflated : s.copied, 0));
  if (g->format == GMX_INGEST_FORMAT_BAM) {
    ing_enqueue_bam(g, si, c.text_len);
    return ing_enqueue_tail(g, si, c);
  }
  const uint32_t n_tiles = c.d_text_len ? g->n_tiles_max : (uint32_t)((ING_CARRY_MAX + (uint64_t)c.text_len + ING_TILE - 1) / ING_TILE);
  hipLaunchKernelGGL(gmx_nl_count_kernel, dim3(n_tiles), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_tiles);
  const uint32_t n_tile_blk = (n_tiles + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK;
  hipLaunchKernelGGL(gmx_tile_scan1_kernel, dim3(n_tile_blk), dim3(64), 0, g->stream, s.d_tiles, n_tiles, s.d_tile_blk);
  hipLaunchKernelGGL(gmx_tile_scan2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_tile_blk, n_tile_blk, s.d_state, g->cap_lines);
  hipLaunchKernelGGL(gmx_nl_mark_kernel, dim3(n_tiles), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_tiles, s.d_tile_blk, s.d_line_end, g->cap_lines);
  const uint32_t fmt = (uint32_t)g->format;
  if (fmt == GMX_INGEST_FORMAT_FASTQ && g->trim_quality) {
    ING_TRY(hipMemsetAsync(s.d_trim, 0, 4 * sizeof(unsigned long long), g->stream));
    hipLaunchKernelGGL(gmx_records_trim_kernel, dim3(2048), dim3(256), 0, g->stream, (const uint8_t *)s.d_text, s.d_state, (const uint32_t *)s.d_line_end, s.d_rec_start,
                       s.d_rec_len, s.d_skip, g->cap_reads, g->trim_quality, g->trim_min_length, s.d_trim);
  } else if (fmt == GMX_INGEST_FORMAT_FASTQ) {
    hipLaunchKernelGGL(gmx_records_kernel, dim3(2048), dim3(256), 0, g->stream, s.d_text, s.d_state, s.d_line_end, s.d_rec_start, s.d_rec_len, s.d_skip, g->cap_reads);
  } else {  // (the chunk's line count is on the device: blocks beyond it leave at once)
    const uint32_t n_line_blk = (uint32_t)(((uint64_t)g->cap_lines + 1 + ING_SCAN_BLOCK - 1) / ING_SCAN_BLOCK);
    hipLaunchKernelGGL(gmx_seq_lines1_kernel, dim3(n_line_blk), dim3(64), 0, g->stream, s.d_text, s.d_state, s.d_line_end, fmt, s.d_line_rec, s.d_line_base, s.d_line_blk);
    hipLaunchKernelGGL(gmx_seq_lines2_kernel, dim3(1), dim3(64), 0, g->stream, s.d_state, s.d_line_end, fmt, s.d_line_blk, s.d_line_base, s.d_rec_line, g->cap_reads);
    hipLaunchKernelGGL(gmx_seq_lines3_kernel, dim3(4096), dim3(256), 0, g->stream, s.d_state, s.d_line_end, s.d_line_rec, s.d_line_base, s.d_line_blk, s.d_rec_line);
    hipLaunchKernelGGL(gmx_seq_records_kernel, dim3(2048), dim3(256), 0, g->stream, s.d_state, s.d_line_end, fmt, s.d_line_base, s.d_rec_line, s.d_rec_start, s.d_rec_len, s.d_skip);
  }
  return ing_enqueue_tail(g, si, c);
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
  for (int i = 0; i < s.n_release; ++i) {  // the mapping kernels that read the slot's planes (gmx_ingest_release_after)
    ING_TRY(hipStreamWaitEvent(g->copy_stream, s.released[i], 0));
    ING_TRY(hipStreamWaitEvent(g->stream, s.released[i], 0));
    ING_TRY(hipStreamWaitEvent(s.inflate_stream, s.released[i], 0));
  }
  s.n_release = 0;
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

// A chunk of BGZF members on its way to the slot (copy stream): the member table checked and translated, the bytes, the table.
static int ing_upload_bgzf(gmx_ingest *g, int slot, const char *who, const uint8_t *compressed, uint64_t n_bytes, const gmx_bgzf_member *members, uint64_t n_members,
                           uint64_t *text_out) {
  if ((!compressed && n_bytes) || (!members && n_members) || n_bytes > g->max_comp || n_members > g->cap_members) {
    gmx_set_error(std::string(who) + ": null argument, or more compressed bytes / members than the ingest was created for");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  uint64_t text = 0;
  for (uint64_t i = 0; i < n_members; ++i) {
    const gmx_bgzf_member &m = members[i];
    if (m.offset + m.size > n_bytes || m.isize > (1u << 16)) {
      gmx_set_error(std::string(who) + ": member " + std::to_string(i) + " lies outside the bytes given, or holds more than 64 KB of text");
      return GMX_EINVAL;
    }
    s.h_members[i] = IngestMember{(uint32_t)m.offset, (uint32_t)m.size, (uint32_t)text, m.isize, m.crc32, 0u};
    text += m.isize;
  }
  if (text > g->max_text) {
    gmx_set_error(std::string(who) + ": the members hold more text than the ingest was created for");
    return GMX_EINVAL;
  }
  // (the bit reader fetches up to 128 words ahead: the staging buffer has slack; the words right behind the data are zeroed)
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_comp, compressed, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipMemsetAsync(reinterpret_cast<uint8_t *>(s.d_comp) + n_bytes, 0, 16, g->copy_stream));
  if (n_members) ING_TRY(hipMemcpyAsync(s.d_members, s.h_members, n_members * sizeof(IngestMember), hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  *text_out = text;
  return GMX_OK;
}
// ... and a chunk of text
static int ing_upload_text(gmx_ingest *g, int slot, const char *who, const uint8_t *text, uint64_t n_bytes) {
  if ((!text && n_bytes) || n_bytes > g->max_text) {
    gmx_set_error(std::string(who) + ": null text, or more text than the ingest was created for");
    return GMX_EINVAL;
  }
  gmx_ingest::Slot &s = g->slot[slot];
  if (n_bytes) ING_TRY(hipMemcpyAsync(s.d_text + ING_CARRY_MAX, text, n_bytes, hipMemcpyHostToDevice, g->copy_stream));
  ING_TRY(hipEventRecord(s.copied, g->copy_stream));
  return GMX_OK;
}

int gmx_ingest_submit_bgzf(gmx_ingest *g, int slot, const uint8_t *compressed, uint64_t n_bytes, const gmx_bgzf_member *members, uint64_t n_members,
                           int final_chunk) try {
  int rc = ing_begin(g, slot, "gmx_ingest_submit_bgzf");
  if (rc) return rc;
  uint64_t text = 0;
  if ((rc = ing_upload_bgzf(g, slot, "gmx_ingest_submit_bgzf", compressed, n_bytes, members, n_members, &text))) return rc;
  IngChunk c;  // inflated here, behind the chunk before on this device
  c.text_len = (uint32_t)text;
  c.inflate_now = c.inflate_status = true;
  c.n_members = (uint32_t)n_members;
  c.final_chunk = final_chunk;
  return ing_enqueue_scan(g, slot, c);
} GMX_GUARD_INT("gmx_ingest_submit_bgzf")

int gmx_ingest_submit_text(gmx_ingest *g, int slot, const uint8_t *text, uint64_t n_bytes, int final_chunk) try {
  int rc = ing_begin(g, slot, "gmx_ingest_submit_text");
  if (rc) return rc;
  if ((rc = ing_upload_text(g, slot, "gmx_ingest_submit_text", text, n_bytes))) return rc;
  IngChunk c;  // text as it is, behind the chunk before on this device
  c.text_len = (uint32_t)n_bytes;
  c.final_chunk = final_chunk;
  return ing_enqueue_scan(g, slot, c);
} GMX_GUARD_INT("gmx_ingest_submit_text")

// bytes of compressed data per piece of the gzip route: GMX_GZ_PIECE (tests cut small files into many), as the first chunk found it
static uint64_t ing_gz_piece_bytes(const gmx_ingest *g) {
  if (g->gz) return g->gz->piece_bytes;
  if (const char *e = getenv("GMX_GZ_PIECE")) return std::min<uint64_t>(std::max<uint64_t>(64, (uint64_t)atoll(e)), 64u << 20);
  return 32u << 10;
}

// The buffers of the gzip route: at its first chunk, and again when a chunk has more pieces than they were made for (the old
// ones are freed: everything that used them ran on `stream`).
static int ing_gz_alloc(gmx_ingest *g, uint32_t n_pieces) {
  std::unique_ptr<gmx_ingest::Gz> z(new gmx_ingest::Gz());
  const uint64_t piece = ing_gz_piece_bytes(g);
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
  const uint64_t piece = ing_gz_piece_bytes(g);
  const uint32_t need = (uint32_t)std::max<uint64_t>(1, (n_own + piece - 1) / piece);
  if ((!g->gz || g->gz->max_pieces < need) && (rc = ing_gz_alloc(g, need))) return rc;
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
  IngChunk c;  // decoded above on `stream`, which holds the text's length; behind the chunk before on this device
  c.d_text_len = &z.d_state->text_len;
  c.inflate_status = true;
  c.final_chunk = final_chunk;
  return ing_enqueue_scan(g, slot, c);
} GMX_GUARD_INT("gmx_ingest_submit_gzip")

int64_t gmx_ingest_gzip_repairs(gmx_ingest *g) try {
  return ing_read_counter(g, g && g->gz ? &g->gz->d_state->repairs : nullptr);
} GMX_GUARD_INT("gmx_ingest_gzip_repairs")

// Chunks dealt over several devices (one ingest per device): the cut record at a chunk's start lies on ANOTHER device, so a chunk
// is uploaded and inflated at once (_deferred) and scanned (gmx_ingest_scan) when the caller has the end of the chunk before —
// gmx_ingest_fetch_tail of that chunk's slot, on its device — which it hands over as host bytes.
int gmx_ingest_submit_bgzf_deferred(gmx_ingest *g, int slot, const uint8_t *compressed, uint64_t n_bytes, const gmx_bgzf_member *members, uint64_t n_members) try {
  if (g && g->format == GMX_INGEST_FORMAT_BAM) return ing_not_bam("gmx_ingest_submit_bgzf_deferred");
  if (g) g->last_slot = -1;  // (nothing is carried on the device in this mode: the slots need not alternate)
  int rc = ing_begin(g, slot, "gmx_ingest_submit_bgzf_deferred");
  if (rc) return rc;
  uint64_t text = 0;
  if ((rc = ing_upload_bgzf(g, slot, "gmx_ingest_submit_bgzf_deferred", compressed, n_bytes, members, n_members, &text))) return rc;
  gmx_ingest::Slot &s = g->slot[slot];
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
  if ((rc = ing_upload_text(g, slot, "gmx_ingest_submit_text_deferred", text, n_bytes))) return rc;
  gmx_ingest::Slot &s = g->slot[slot];
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
  IngChunk c;  // uploaded (and inflating) since the _deferred call; the cut record comes from the caller
  c.text_len = s.deferred_text;
  c.inflate_status = s.deferred_inflate;
  c.carry_on_device = false;
  c.host_carry = (uint32_t)n_carry;
  c.final_chunk = final_chunk;
  return ing_enqueue_scan(g, slot, c);
} GMX_GUARD_INT("gmx_ingest_scan")

// bytes [from, from + n) of the slot's text buffer, both taken from the chunk's state: their number (out null), or the bytes
static int64_t ing_fetch_range(gmx_ingest *g, int slot, const char *who, uint32_t IngestState::*from, uint32_t IngestState::*n, uint8_t *out, uint64_t cap) {
  if (!g || slot < 0 || slot >= GMX_INGEST_SLOTS || g->slot[slot].in_flight) {
    gmx_set_error(std::string(who) + ": null ingest, bad slot, or the slot's chunk is still in flight");
    return GMX_EINVAL;
  }
  const IngestState &st = *g->slot[slot].h_state;
  if (!out) return (int64_t)(st.*n);
  if (cap < st.*n) {
    gmx_set_error(std::string(who) + ": buffer too small");
    return GMX_EINVAL;
  }
  if (st.*n && (hipSetDevice(g->device) != hipSuccess || hipMemcpy(out, g->slot[slot].d_text + st.*from, st.*n, hipMemcpyDeviceToHost) != hipSuccess)) {
    gmx_set_error(std::string(who) + ": hipMemcpy failed");
    return GMX_EHIP;
  }
  return (int64_t)(st.*n);
}

int64_t gmx_ingest_fetch_tail(gmx_ingest *g, int slot, uint8_t *out, uint64_t cap) try {
  return ing_fetch_range(g, slot, "gmx_ingest_fetch_tail", &IngestState::consumed, &IngestState::tail_len, out, cap);
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
  const int i = s.n_release ? 1 : 0;  // (a second stream behind the same chunk; a third call records the second event again)
  ING_TRY(hipEventRecord(s.released[i], (hipStream_t)hip_stream));
  s.n_release = i + 1;
  return GMX_OK;
} GMX_GUARD_INT("gmx_ingest_release_after")

int64_t gmx_ingest_fetch_text(gmx_ingest *g, int slot, uint8_t *out, uint64_t cap) try {
  return ing_fetch_range(g, slot, "gmx_ingest_fetch_text", &IngestState::text_start, &IngestState::text_len, out, cap);
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

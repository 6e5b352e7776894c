// The device feed of `gram`: reads files decoded, scanned and packed on the GPU (include/gmx.h gmx_ingest_*, gmx_ingest.hip).
// A piece of gram_main.cpp, included there once inside its namespace: it uses die, GMX_CHECK, HostBuf, parallel_for, feed_trace,
// g_feed, SeqReader and g_reads_format of that file. DESIGN.md §11.
// One pipeline behind every route: a file's chunks go to the device ahead of the one being waited for, each chunk's status is
// turned into a verdict (chunk_verdict), a chunk that passes is handed to `on_chunk(result, k, slot)` in file order — engine
// k's ingest holds its reads in HBM; the callback must enqueue what reads them and call gmx_ingest_release_after. The routes
// differ in where a chunk's bytes come from and in how far ahead they submit: feed_chunks (one engine: BGZF members, plain text,
// plain gzip, three submission policies) and feed_chunks_dealt (several engines: BGZF members, text slices). Every route returns
//          0  the whole file was delivered
//          1  declined before anything was delivered (not what the route reads, or not four-line FASTQ: the caller's other readers decide)
//          2  a chunk could not be decoded after `delivered` reads had been: the caller re-reads the file on the host, which
//             either reports the damage or — a defect of the device decoder — delivers the rest

// ---- BGZF members ----------------------------------------------------------------------------------------------------------
// A file that is BGZF members from its first byte to its last (bgzip, htslib, BCL Convert) is handed to the device as it
// lies in the page cache: the member table is walked here (18 bytes per member), the deflate data of a few thousand members
// at a time is copied into page-locked memory by all threads and uploaded, and HIP kernels inflate it, check every member's
// CRC-32, find the records and pack the bases — the host inflates nothing (sixteen cores manage 32-48 M reads/s of BGZF; the
// mapping kernels take 2 400 M).
static bool bgzf_member_at(const unsigned char *in, size_t size, size_t at, gmx_bgzf_member *m, size_t *next) {
  auto le16 = [](const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; };
  auto le32 = [](const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; };
  if (at + 18 > size) return false;
  const unsigned char *p = in + at;
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return false;
  const uint32_t xlen = le16(p + 10);
  if (at + 12 + xlen > size) return false;
  uint32_t bsize = 0;
  bool found = false;
  for (uint32_t x = 0; x + 4 <= xlen;) {
    const unsigned char *f = p + 12 + x;
    const uint32_t slen = le16(f + 2);
    if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) {
      bsize = le16(f + 4) + 1;
      found = true;
    }
    x += 4 + slen;
  }
  if (!found || bsize < 12 + xlen + 8 || at + bsize > size) return false;
  m->offset = at + 12 + xlen;
  m->size = bsize - 12 - xlen - 8;
  m->crc32 = le32(p + bsize - 8);
  m->isize = le32(p + bsize - 4);
  m->reserved = 0;
  *next = at + bsize;
  return m->isize <= 65536u;
}

// ---- the ingests and their staging buffers ---------------------------------------------------------------------------------
struct DeviceFeed {  // one per engine: the ingest object and its page-locked staging, sized by the largest file seen
  gmx_ingest *ing = nullptr;
  uint64_t max_text = 0;
  int device = 0;
  HostBuf<uint8_t> stage[4];  // (BGZF uses three: chunk i + 2's bytes are staged while chunks i and i + 1 are on the device; plain text four: ingest_text_file)
  ~DeviceFeed() {
    if (ing) gmx_ingest_destroy(ing);
  }
};
static DeviceFeed g_device_feed;                             // the first (or only) engine's
static std::vector<std::unique_ptr<DeviceFeed>> g_more_feeds;  // the other engines' (several GPUs: chunks dealt round)
static DeviceFeed &device_feed(size_t k) { return k == 0 ? g_device_feed : *g_more_feeds[k - 1]; }

// the ingest object and its staging buffers ahead of the first reads file (called beside the index load: device memory for a
// chunk and two page-locked buffers take 30 ms to come by; gmx_ingest_create selects the device itself)
static void device_feed_prepare(int device, uint64_t want_text, uint64_t stage_bytes, DeviceFeed *which = nullptr) {
  DeviceFeed &df = which ? *which : g_device_feed;
  if (!df.ing || df.max_text < want_text || df.device != device) {
    if (df.ing) gmx_ingest_destroy(df.ing);
    df.ing = nullptr;
    df.max_text = 0;
    if (gmx_ingest_create(device, want_text, &df.ing) != GMX_OK) return;
    df.max_text = want_text;
    df.device = device;
  }
  for (auto &st : df.stage)
    if (st.size() < stage_bytes) st.resize(stage_bytes);
}
// The ingests of engines 0 .. n - 1 made (or kept) for chunks of want_text, reset and set to the file's format
// (g_reads_format: every route goes through here, so the caller sets it once per file). false: an ingest could not be made,
// or holds fewer than need_compressed bytes of deflate data — the route declines.
static bool device_feeds_ready(const int *devs, size_t n, uint64_t want_text, uint64_t stage_bytes = 0, uint64_t need_compressed = 0) {
  while (g_more_feeds.size() + 1 < n) g_more_feeds.emplace_back(new DeviceFeed());
  for (size_t k = 0; k < n; ++k) {
    DeviceFeed &df = device_feed(k);
    device_feed_prepare(devs[k], want_text, stage_bytes, &df);
    if (!df.ing || (need_compressed && gmx_ingest_max_compressed(df.ing) < need_compressed)) return false;
    GMX_CHECK(gmx_ingest_reset(df.ing));
    GMX_CHECK(gmx_ingest_set_format(df.ing, g_reads_format));
    if (g_trim_quality) GMX_CHECK(gmx_ingest_set_quality_trim(df.ing, g_trim_quality, g_trim_min_length));  // --trim_quality (BAM never comes here with it)
  }
  return true;
}
static unsigned feed_threads(int threads) { return (unsigned)std::max(1, std::min(threads, 64)); }

// ---- chunk sizes -----------------------------------------------------------------------------------------------------------
static uint64_t device_feed_members() {
  uint64_t k = 7168 * g_ingest_member_scale;  // one round of the wavefronts an MI355X holds of gmx_inflate_kernel (28 per CU)
  if (const char *e = getenv("GMX_INGEST_MEMBERS")) k = std::max<uint64_t>(1, (uint64_t)atoll(e));
  return k;
}
static uint64_t device_feed_text_for(uint64_t file_text) {
  return std::min<uint64_t>(std::max<uint64_t>(std::min<uint64_t>(file_text, device_feed_members() * 65536ull), 1u << 16) + (1u << 16), 3ull << 30);
}
static uint64_t device_feed_text_chunk(size_t scale = 0) {
  uint64_t c = (128ull << 20) * (scale ? scale : std::min<size_t>(g_block_scale, 4));  // (nested PRGs: larger launches, see g_block_scale; 128 MB: 29-33 ms per 1.26 GB where 64 MB chunks take 34-40)
  if (const char *e = getenv("GMX_TEXT_CHUNK")) c = std::max<uint64_t>(64, (uint64_t)atoll(e));
  return std::min<uint64_t>(c, (3ull << 30) - (1u << 20));
}
static uint64_t device_feed_text_room(uint64_t chunk) { return std::max<uint64_t>(chunk, 1u << 16) + (1u << 16); }  // a text chunk and the record carried into it
static uint64_t device_feed_gz_chunk() {
  uint64_t c = 32ull << 20;
  if (const char *e = getenv("GMX_GZ_CHUNK")) c = std::max<uint64_t>(64, (uint64_t)atoll(e));
  return std::min<uint64_t>(c, 256ull << 20);
}

// ---- which route takes a file ----------------------------------------------------------------------------------------------
// Which reader takes a plain FASTQ (measured on the GPU boxes, configs[1], 4 M x 150 bp = 1.26 GB in the page cache, parse + map;
// profiles/round6/cli_text_feed_by_threads.txt): the device route moves 316 B per read over the host link and is bound by it —
// 28-33 ms = 120-140 M reads/s from 2 host threads on, 67 M with ONE (one core copies 21 GB/s out of the page cache) — while the
// host parser sends 40 B per read and scales with the cores: 24 M reads/s on 1 thread, 35-45 M on 2-4, 52-82 M on 8, 75-102 M on 16,
// 140-165 M on 32, 140-215 M on 64. So: the device route below 32 host threads (`--max_threads` defaults to 1 in the reference's
// front-end: 2.8 x), the host parser from 32 threads on. GMX_DEVICE_FASTQ=1 / GMX_HOST_FASTQ=1 force either.
static bool plain_fastq_on_device(int max_threads, size_t n_engines) {
  if (getenv("GMX_HOST_FASTQ")) return false;
  // FASTA / one read per line: no parallel host parser exists for them (parse_fastq_file declines), the alternative is the
  // general reader on ONE thread: the device route at every thread count
  if (g_reads_format != GMX_INGEST_FORMAT_FASTQ) return true;
  if (g_trim_quality) return true;  // --trim_quality: the parallel host parser never sees the quality line, the record scan trims
  if (const char *e = getenv("GMX_DEVICE_FASTQ")) return atoi(e) != 0;
  (void)n_engines;  // (several engines: the same rule — the chunks are then dealt over the engines' ingests, ingest_text_file_dealt; measured
                    //  only with several engines on ONE GPU, tools/feed_x8.py, where it has nothing to gain)
  return max_threads < 32;
}
static uint64_t fstat_ok_size(const std::string &path) {
  struct stat sb;
  return stat(path.c_str(), &sb) == 0 && S_ISREG(sb.st_mode) ? (uint64_t)sb.st_size : 0;
}
// the first three bytes of a regular file of at least min_size bytes, and its size (looked at only where the probe says yes)
static bool file_head(const std::string &path, off_t min_size, unsigned char *h, uint64_t *size_out) {
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  struct stat sb;
  const bool ok = fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size >= min_size && pread(fd, h, 3, 0) == 3;
  close(fd);
  if (ok && size_out) *size_out = (uint64_t)sb.st_size;
  return ok;
}
static bool looks_like_plain_fastq(const std::string &path, uint64_t *size_out) {
  unsigned char h[3];
  // (FASTA / one read per line, as detect_reads_format found: any first byte — blank lines may lead — but gzip's)
  return file_head(path, 4, h, size_out) && (g_reads_format == GMX_INGEST_FORMAT_FASTQ ? h[0] == '@' : !(h[0] == 0x1f && h[1] == 0x8b));
}
static bool looks_like_gzip(const std::string &path, uint64_t *size_out) {
  unsigned char h[3];
  return file_head(path, 18, h, size_out) && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8;
}

// ---- a file's bytes into page-locked memory --------------------------------------------------------------------------------
// bytes [at, at + n) of the file into dst, every thread its slice (page cache -> page-locked memory); false: a read failed
static bool pread_parallel(int fd, uint64_t at, uint8_t *dst, size_t n, unsigned T) {
  std::atomic<bool> bad{false};
  parallel_for(T, [&](unsigned t) {
    size_t lo = n * t / T;
    const size_t hi = n * (t + 1) / T;
    while (lo < hi) {
      const ssize_t got = pread(fd, dst + lo, hi - lo, (off_t)(at + lo));
      if (got <= 0) {
        bad.store(true);
        return;
      }
      lo += (size_t)got;
    }
  });
  return !bad.load();
}
struct ReadFile {  // an open file read with pread
  int fd;
  explicit ReadFile(const std::string &path) : fd(open(path.c_str(), O_RDONLY)) {}
  ReadFile(const ReadFile &) = delete;
  ~ReadFile() {
    if (fd >= 0) close(fd);
  }
  bool copy(uint64_t lo, uint64_t hi, uint8_t *dst, unsigned T) const { return pread_parallel(fd, lo, dst, (size_t)(hi - lo), T); }
};
struct MappedFile {  // a file of at least min_size bytes mapped read-only: the page cache's own pages
  const unsigned char *in = nullptr;
  size_t size = 0;
  MappedFile(const std::string &path, size_t min_size) {
    const ReadFile f(path);
    struct stat sb;
    if (f.fd < 0 || fstat(f.fd, &sb) != 0 || (size_t)sb.st_size < min_size) return;
    void *mp = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE | MAP_NORESERVE, f.fd, 0);
    if (mp == MAP_FAILED) return;
    in = static_cast<const unsigned char *>(mp);
    size = (size_t)sb.st_size;
  }
  MappedFile(const MappedFile &) = delete;
  ~MappedFile() {
    if (in) munmap(const_cast<unsigned char *>(in), size);
  }
  void copy(size_t lo, size_t hi, HostBuf<uint8_t> &st, unsigned T) const {  // (the compressed bytes: 5 ms a chunk)
    const size_t n = hi - lo;
    st.resize(n + 64);
    parallel_for(T, [&](unsigned t) {
      const size_t a = n * t / T, b = n * (t + 1) / T;
      if (b > a) memcpy(st.data() + a, in + lo + a, b - a);
    });
  }
};

// ---- what a chunk's status means -------------------------------------------------------------------------------------------
enum class FeedRoute { Bgzf, Gzip, Text };
// 0 go on, else the route's return value (1 declined, 2 the host reader takes over) — or the end of the run:
//   route        status                                   nothing delivered      reads delivered
//   gzip         any                                      2                      2     (the host reader reports real damage itself)
//   BGZF, BAM    any                                      2                      2     (the host reader names a malformed record)
//   BGZF         BAD_MEMBER / BAD_CRC                     2                      2
//   BGZF         TOO_MANY_LINES, none of the above        1                      2     (lines of a few bytes: more records than the ingest has room for)
//   BGZF         none of the three ("irregular")          1                      FASTQ: fatal; FASTA / one read per line: 2
//   text         BAD_RECORD ("irregular")                 1                      FASTQ: fatal; FASTA / one read per line: 2
//   text         anything else                            1                      2
// "irregular": the text itself is not what its format says — the host's fast path would say the same of a four-line FASTQ.
static int chunk_verdict(FeedRoute route, uint32_t status, uint64_t delivered, const std::string &path) {
  if (!status) return 0;
  if (route == FeedRoute::Gzip || (route == FeedRoute::Bgzf && g_reads_format == GMX_INGEST_FORMAT_BAM)) return 2;
  const bool bgzf = route == FeedRoute::Bgzf;
  const bool irregular = bgzf ? !(status & (GMX_INGEST_BAD_MEMBER | GMX_INGEST_BAD_CRC | GMX_INGEST_TOO_MANY_LINES)) : (status & GMX_INGEST_BAD_RECORD) != 0;
  if (irregular && delivered) {
    if (g_reads_format != GMX_INGEST_FORMAT_FASTQ) return 2;  // (the general reader takes over and skips what was mapped)
    die("gram: " + path + ": irregular FASTQ record after the first " + std::to_string(delivered) +
        " reads (multi-line or blank lines); " + (bgzf ? "decompress and reformat" : "reformat") + ", or use a four-line FASTQ");
  }
  const bool damaged = bgzf && (status & (GMX_INGEST_BAD_MEMBER | GMX_INGEST_BAD_CRC));
  return delivered == 0 && !damaged ? 1 : 2;
}
// Test hook GMX_INGEST_TEST_FAIL_CHUNK=i (tests/test_ingest.py, test_ingest_gzip.py): the device "gives up" on chunk i — a member
// it would not decode (BGZF, gzip), more records than the ingest has room for (text). Read once per file.
struct FailHook {
  const char *env = getenv("GMX_INGEST_TEST_FAIL_CHUNK");
  size_t chunk = env ? (size_t)atoll(env) : ~(size_t)0;
  void apply(FeedRoute route, size_t ci, gmx_ingest_result &res) const {
    if (ci == chunk) res.status |= route == FeedRoute::Text ? GMX_INGEST_TOO_MANY_LINES : GMX_INGEST_BAD_MEMBER;
  }
};

// ---- one engine ------------------------------------------------------------------------------------------------------------
// The loop of every single-engine route: chunk ci takes slot ci % 3 of the ingest. `ahead(ci)` makes sure chunk ci is
// submitted, and as many behind it as the route's policy allows: 1 it is, 0 the file has no chunk ci, -1 a chunk's bytes could
// not be read. `n_submitted` is the source's count of chunks submitted so far.
template <class Ahead, class OnChunk>
int feed_chunks(gmx_ingest *ing, FeedRoute route, const char *trace_done, const std::string &path, Ahead ahead, const size_t &n_submitted, OnChunk on_chunk,
                uint64_t *delivered) {
  const FailHook hook;
  auto drain = [&](size_t from) {  // (the chunks in flight: let them finish before the slots are reused)
    for (size_t cj = from; cj < n_submitted; ++cj) {
      gmx_ingest_result drop;
      GMX_CHECK(gmx_ingest_wait(ing, (int)(cj % 3), &drop));
    }
  };
  for (size_t ci = 0;; ++ci) {
    const int there = ahead(ci);
    if (there == 0) return 0;
    if (there < 0) {  // (then the host reader reports the file)
      drain(ci);
      return *delivered == 0 ? 1 : 2;
    }
    gmx_ingest_result res;
    GMX_CHECK(gmx_ingest_wait(ing, (int)(ci % 3), &res));
    feed_trace(trace_done);
    hook.apply(route, ci, res);
    if (res.status) {
      drain(ci + 1);
      return chunk_verdict(route, res.status, *delivered, path);
    }
    on_chunk(res, (size_t)0, (int)(ci % 3));
    *delivered += res.n_reads;
  }
}

template <class OnChunk>
int ingest_bgzf_file(const std::string &path, int threads, int device, OnChunk on_chunk, uint64_t *delivered) {
  *delivered = 0;
  const MappedFile file(path, 28);
  if (!file.in) return 1;
  const unsigned char *in = file.in;
  const size_t size = file.size;
  // The member table is walked a chunk at a time, beside the device (round 5: the whole table first cost 7 ms of a 22 000-member file
  // before the first byte went up). Every byte of the file must belong to a BGZF member: a file that stops being BGZF behind chunks
  // already delivered is handed to the host reader, which drops what was mapped (return value 2).
  {  // not BGZF at its first byte: declined BEFORE the ingest is sized for it (round 6: a plain FASTQ of 1.26 GB had the ingest the
     // prewarm thread made for its text chunks thrown away and one for 470 MB chunks made here — 40 ms — just to be declined)
    gmx_bgzf_member m0;
    size_t next0;
    if (!bgzf_member_at(in, size, 0, &m0, &next0)) return 1;
  }
  if (!device_feeds_ready(&device, 1, device_feed_text_for((uint64_t)size * 6))) return 1;  // (as the call beside the index load sized it)
  DeviceFeed &df = g_device_feed;
  gmx_ingest *ing = df.ing;
  const bool bam = g_reads_format == GMX_INGEST_FORMAT_BAM;
  if (bam) {  // the header's length in the file's text: zlib inflates the file's head (a header that cannot be read: the host reader says why)
    SeqReader head(path);
    if (!head.is_bam()) return 1;
    GMX_CHECK(gmx_ingest_set_bam_header(ing, head.bam_header_bytes()));
  }
  // (a chunk holds at most what the ingest's member table holds: a file of many tiny members must not be refused by the submit)
  const uint64_t kMembers = std::min<uint64_t>(device_feed_members(), gmx_ingest_max_members(ing));
  const uint64_t max_text = gmx_ingest_max_text(ing), max_comp = gmx_ingest_max_compressed(ing);
  struct Chunk {
    std::vector<gmx_bgzf_member> rel;  // its members, offsets from lo
    size_t lo = 0, hi = 0;             // file bytes their deflate data spans
  };
  size_t walk_at = 0;
  auto skip_empty = [&]() -> bool {  // to the next member that holds text; false: the bytes there are no BGZF member
    while (walk_at < size) {
      gmx_bgzf_member m;
      size_t next;
      if (!bgzf_member_at(in, size, walk_at, &m, &next)) return false;
      if (m.isize) break;
      walk_at = next;  // (empty members — the EOF marker — hold nothing)
    }
    return true;
  };
  // the next chunk of members: at most kMembers, and what the ingest has room for. 1: a chunk, 0: the file's end, -1: not BGZF
  auto next_chunk = [&](Chunk &c) -> int {
    c.rel.clear();
    c.lo = c.hi = 0;
    uint64_t text = 0;
    while (walk_at < size) {
      gmx_bgzf_member m;
      size_t next;
      if (!bgzf_member_at(in, size, walk_at, &m, &next)) return -1;
      if (m.isize) {
        if (c.rel.empty()) c.lo = (size_t)m.offset;
        if (c.rel.size() >= kMembers || text + m.isize > max_text || m.offset + m.size - c.lo > max_comp) break;
        text += m.isize;
        c.hi = (size_t)(m.offset + m.size);
        m.offset -= c.lo;
        c.rel.push_back(m);
      }
      walk_at = next;
    }
    if (c.rel.empty()) return walk_at < size ? -1 : 0;  // (a member the ingest has no room for: cannot happen with <= 64 KB members)
    return skip_empty() ? 1 : -1;                        // (so that walk_at == size tells a chunk it is the file's last)
  };
  const unsigned T = feed_threads(threads);
  // Chunk i + 2's bytes are staged (page cache -> page-locked memory, 5 ms a chunk) and submitted while chunks i and i + 1 are on the
  // device (the ingest's three slots): the device never waits for the host's memcpy
  // (round 5: staged inside the submit, the copy sat between a chunk's result and the next chunk's upload — a GPU idle for 6 ms of
  // every 13). Three staging buffers: the one chunk i + 2 takes was chunk i - 1's, whose upload is long done (it has been waited for).
  Chunk ring[3];
  bool last_of_file[3] = {false, false, false};
  size_t n_staged = 0;  // chunks walked and staged so far
  bool at_end = false, bad_walk = false;
  auto stage = [&]() -> bool {  // the next chunk, into slot n_staged % 3; false: there is none
    if (at_end || bad_walk) return false;
    Chunk &c = ring[n_staged % 3];
    const int rc = next_chunk(c);
    if (rc <= 0) {
      at_end = rc == 0;
      bad_walk = rc < 0;
      return false;
    }
    last_of_file[n_staged % 3] = walk_at >= size;
    file.copy(c.lo, c.hi, df.stage[n_staged % 3], T);
    ++n_staged;
    return true;
  };
  size_t n_submitted = 0;
  auto submit = [&]() {  // chunk n_submitted (staged)
    const size_t ci = n_submitted;
    const Chunk &c = ring[ci % 3];
    GMX_CHECK(gmx_ingest_submit_bgzf(ing, (int)(ci % 3), df.stage[ci % 3].data(), c.hi - c.lo, c.rel.data(), c.rel.size(), last_of_file[ci % 3] ? 1 : 0));
    ++n_submitted;
    feed_trace("chunk submitted to the device");
  };
  if (!skip_empty()) return 1;
  if (!stage()) return bad_walk ? 1 : 0;  // (0: no reads at all)
  submit();
  feed_trace("first chunk on its way; the member table is walked beside the device");
  if (stage()) submit();
  // chunk ci + 2 goes to the device BEFORE chunk ci is waited for (three slots: its slot is chunk ci - 1's, waited for and handed to
  // the engine): two inflate kernels are queued behind the one in flight, and a kernel's last wavefronts never have the GPU alone
  auto ahead = [&](size_t ci) -> int {
    if (ci >= n_submitted) return 0;
    if (n_staged == n_submitted) stage();
    if (n_staged > n_submitted) submit();
    return 1;
  };
  const int rc = feed_chunks(ing, FeedRoute::Bgzf, bam ? "BAM chunk chained and packed" : "chunk decoded", path, ahead, n_submitted, on_chunk, delivered);
  if (rc == 0 && bad_walk) return *delivered == 0 && !bam ? 1 : 2;  // bytes that are no BGZF member behind the chunks delivered: the host reader's
  return rc;
}

// ---- plain (uncompressed) four-line FASTQ through the same device chain (round 6) -----------------------------------------
// The reference reads every text format through one host reader (include/sequence_read/seqread.hpp:94-180, seq_file.h:626-633,
// quasimap.cpp:65-76). Until round 6 `gram` took the device route for BGZF only and parsed a plain FASTQ on the host: 42 M
// reads/s parse + map at configs[1], 3.5 x slower than the same reads bgzipped. Now the file's bytes go up as they are: all
// threads pread their slices of a chunk from the page cache into page-locked memory (ONE pass over the text on the host, no
// parsing), the chunk is uploaded (gmx_ingest_submit_text) and gmx_nl_* / gmx_records / gmx_fq_pack find the records and pack the
// bases in HBM; a record cut by a chunk's end is carried into the next chunk on the device. Bound: the host link at ~316 B per
// 150-base read (measured 120-140 M reads/s; the link's 55 GB/s would be 175 M). Whether a file takes this route or the host parser:
// plain_fastq_on_device() above.
template <class OnChunk>
int ingest_text_file(const std::string &path, int threads, int device, OnChunk on_chunk, uint64_t *delivered) {
  *delivered = 0;
  uint64_t size = 0;
  if (!looks_like_plain_fastq(path, &size)) return 1;
  const ReadFile f(path);
  if (f.fd < 0) return 1;
  const uint64_t chunk = std::min<uint64_t>(device_feed_text_chunk(), size);
  if (!device_feeds_ready(&device, 1, device_feed_text_room(chunk))) return 1;
  DeviceFeed &df = g_device_feed;
  gmx_ingest *ing = df.ing;
  const unsigned T = feed_threads(threads);
  const size_t n_chunks = (size_t)((size + chunk - 1) / chunk);
  auto bytes_of = [&](size_t ci) { return (size_t)std::min<uint64_t>(chunk, size - (uint64_t)ci * chunk); };
  // A thread of its own reads the chunks ahead into four page-locked buffers (round 6: read, submit, wait and map in turn on one
  // thread cost 1.55 ms per 64 MB chunk of which 1.25 were the read — the reads now run back to back). Buffer k % 4 is free for
  // chunk k once chunk k - 4 has been waited for (its upload is over).
  constexpr size_t NB = 4;
  HostBuf<uint8_t> *const ring = df.stage;  // (sized beside the index load: device_feed_prepare; page-locking 4 x 64 MB takes 30 ms)
  struct Reader {
    std::mutex m;
    std::condition_variable cv;
    size_t staged = 0, waited = 0;  // chunks read so far / chunks the consumer is done with
    bool failed = false, stop = false;
    std::thread th;
    ~Reader() {
      {
        std::lock_guard<std::mutex> lk(m);
        stop = true;
      }
      cv.notify_all();
      if (th.joinable()) th.join();
    }
  } rd;
  for (size_t b = 0; b < std::min(NB, n_chunks); ++b) ring[b].resize(bytes_of(0) + 64);
  rd.th = std::thread([&]() {
    for (size_t k = 0; k < n_chunks; ++k) {
      {
        std::unique_lock<std::mutex> lk(rd.m);
        rd.cv.wait(lk, [&] { return rd.stop || k < rd.waited + NB; });
        if (rd.stop) return;
      }
      const double t_read = now_s();
      const bool ok = f.copy((uint64_t)k * chunk, (uint64_t)k * chunk + bytes_of(k), ring[k % NB].data(), T);
      g_feed.read_s += now_s() - t_read;
      feed_trace("  text chunk read into page-locked memory");
      {
        std::lock_guard<std::mutex> lk(rd.m);
        if (!ok) rd.failed = true;
        rd.staged = k + 1;
      }
      rd.cv.notify_all();
      if (!ok) return;
    }
  });
  auto staged = [&](size_t k, bool block) -> int {  // 1: chunk k is read, 0: not yet (block = false), -1: its read failed
    std::unique_lock<std::mutex> lk(rd.m);
    if (block) rd.cv.wait(lk, [&] { return rd.staged > k || rd.failed; });
    if (rd.staged > k) return 1;
    return rd.failed ? -1 : 0;
  };
  size_t n_submitted = 0;
  auto submit = [&]() {
    const size_t ci = n_submitted;
    GMX_CHECK(gmx_ingest_submit_text(ing, (int)(ci % 3), ring[ci % NB].data(), bytes_of(ci), ci + 1 == n_chunks ? 1 : 0));
    ++n_submitted;
    feed_trace("text chunk submitted to the device");
  };
  auto ahead = [&](size_t ci) -> int {
    if (ci) {  // (the chunks before ci have been waited for: their buffers are the reader's again)
      {
        std::lock_guard<std::mutex> lk(rd.m);
        rd.waited = ci;
      }
      rd.cv.notify_all();
    }
    if (ci >= n_chunks) return 0;
    if (n_submitted <= ci) {  // this chunk itself: wait for its bytes
      if (staged(ci, true) < 0) return -1;
      submit();
    }
    while (n_submitted < std::min(n_chunks, ci + 3) && staged(n_submitted, false) == 1) submit();  // the two behind it, when they are there
    return 1;
  };
  return feed_chunks(ing, FeedRoute::Text, "text chunk scanned and packed", path, ahead, n_submitted, on_chunk, delivered);
}

// A PLAIN gzip file (one deflate stream per member: gzip, pigz, ENA / SRA downloads) decoded on the device
// (gmx_ingest_submit_gzip): chunks of GMX_GZ_CHUNK compressed bytes (default 32 MB) with 1 MB of the file behind
// each as look-ahead, read into page-locked buffers and submitted with two chunks on the device. One engine only: the deflate
// stream's window and position live in that engine's ingest. Returns 1: not gzip.
template <class OnChunk>
int ingest_gzip_file(const std::string &path, int threads, int device, OnChunk on_chunk, uint64_t *delivered) {
  *delivered = 0;
  uint64_t size = 0;
  if (!looks_like_gzip(path, &size)) return 1;
  const ReadFile f(path);
  if (f.fd < 0) return 1;
  const uint64_t chunk = std::min<uint64_t>(device_feed_gz_chunk(), size), look = 1u << 20;
  // text room for 8:1 (FASTQ compresses 3-5 fold; a chunk that inflates further comes back with GMX_INGEST_GZ_TEXT_LIMIT)
  if (!device_feeds_ready(&device, 1, std::max<uint64_t>(2 * (chunk + look), std::min<uint64_t>(8 * chunk, 3ull << 30)), chunk + look + 64, chunk + look)) return 1;
  DeviceFeed &df = g_device_feed;
  gmx_ingest *ing = df.ing;
  const unsigned T = feed_threads(threads);
  const size_t n_chunks = (size_t)((size + chunk - 1) / chunk);
  size_t n_submitted = 0;
  auto submit = [&]() -> bool {
    const size_t ci = n_submitted;
    const uint64_t at = (uint64_t)ci * chunk, own = std::min<uint64_t>(chunk, size - at);
    const bool final_chunk = ci + 1 == n_chunks;
    const uint64_t n = final_chunk ? own : std::min<uint64_t>(own + look, size - at);
    const double t_read = now_s();
    if (!f.copy(at, at + n, df.stage[ci % 3].data(), T)) return false;
    g_feed.read_s += now_s() - t_read;
    GMX_CHECK(gmx_ingest_submit_gzip(ing, (int)(ci % 3), df.stage[ci % 3].data(), n, own, final_chunk ? 1 : 0));
    ++n_submitted;
    feed_trace("gzip chunk submitted to the device");
    return true;
  };
  auto ahead = [&](size_t ci) -> int {
    if (ci >= n_chunks) return 0;
    while (n_submitted < std::min(n_chunks, ci + 2))  // this chunk and the one behind it on the device
      if (!submit()) return -1;
    return 1;
  };
  return feed_chunks(ing, FeedRoute::Gzip, "gzip chunk decoded, scanned and packed", path, ahead, n_submitted, on_chunk, delivered);
}

// ---- several engines (`--devices`) --------------------------------------------------------------------------
// One ingest per engine, the file's chunks dealt round: chunk ci goes to engine ci % N, slot (ci / N) & 1. Every chunk is
// uploaded (and, BGZF, inflated) ahead, two per engine in flight; the chunks are scanned in file order, each with the cut
// record of the chunk before — which lies on another device — handed over through the host (a few hundred bytes).
// `stage(ci)` brings chunk ci's bytes into its engine's staging buffer and submits it deferred; false: the bytes could not be
// read. Nothing of such a chunk goes to a device: the chunks in flight are dropped and the host reader reports the file.
template <class Stage, class OnChunk>
int feed_chunks_dealt(size_t N, size_t n_chunks, FeedRoute route, const char *trace_scanned, const std::string &path, Stage stage, OnChunk on_chunk,
                      uint64_t *delivered) {
  const FailHook hook;
  auto ingest_of = [&](size_t ci) { return device_feed(ci % N).ing; };
  auto slot_of = [&](size_t ci) { return (int)((ci / N) & 1); };
  size_t submitted = 0;
  auto drain = [&](size_t from) {  // (chunks uploaded ahead: scanned with nothing and dropped, so that their slots are free again)
    for (size_t cj = from; cj < submitted; ++cj) {
      gmx_ingest_result drop;
      GMX_CHECK(gmx_ingest_scan(ingest_of(cj), slot_of(cj), nullptr, 0, 0));
      GMX_CHECK(gmx_ingest_wait(ingest_of(cj), slot_of(cj), &drop));
    }
  };
  auto unread = [&](size_t from) {
    drain(from);
    return *delivered == 0 ? 1 : 2;
  };
  for (; submitted < std::min(n_chunks, 2 * N); ++submitted)
    if (!stage(submitted)) return unread(0);
  std::vector<uint8_t> tail;
  for (size_t ci = 0; ci < n_chunks; ++ci) {
    gmx_ingest *ing = ingest_of(ci);
    GMX_CHECK(gmx_ingest_scan(ing, slot_of(ci), tail.data(), tail.size(), ci + 1 == n_chunks ? 1 : 0));
    gmx_ingest_result res;
    GMX_CHECK(gmx_ingest_wait(ing, slot_of(ci), &res));
    feed_trace(trace_scanned);
    hook.apply(route, ci, res);
    if (res.status) {
      drain(ci + 1);
      return chunk_verdict(route, res.status, *delivered, path);
    }
    tail.resize(res.tail_bytes);
    if (res.tail_bytes && gmx_ingest_fetch_tail(ing, slot_of(ci), tail.data(), tail.size()) < 0) die(std::string("gram: ") + gmx_last_error());
    on_chunk(res, ci % N, slot_of(ci));
    *delivered += res.n_reads;
    if (submitted < n_chunks) {  // (its slot: chunk submitted - 2 N, waited for and handed on two rounds ago)
      if (!stage(submitted)) return unread(ci + 1);
      ++submitted;
    }
  }
  return 0;
}

// BGZF members as the dealt source: the member table is walked up front (a file that is not BGZF to its last byte is declined
// before anything goes up), chunks of at most GMX_INGEST_MEMBERS members.
template <class OnChunk>
int ingest_bgzf_file_dealt(const std::string &path, int threads, const std::vector<int> &devs, OnChunk on_chunk, uint64_t *delivered) {
  *delivered = 0;
  const size_t N = devs.size();
  const MappedFile file(path, 28);
  if (!file.in) return 1;
  std::vector<gmx_bgzf_member> members;
  members.reserve(file.size / 16000 + 16);
  uint64_t file_text = 0;
  for (size_t at = 0; at < file.size;) {
    gmx_bgzf_member m;
    size_t next;
    if (!bgzf_member_at(file.in, file.size, at, &m, &next)) return 1;
    if (m.isize) members.push_back(m);
    file_text += m.isize;
    at = next;
  }
  if (!device_feeds_ready(devs.data(), N, device_feed_text_for(file_text))) return 1;
  feed_trace("ingests of all engines ready");
  gmx_ingest *ing0 = device_feed(0).ing;
  const uint64_t max_text = gmx_ingest_max_text(ing0), max_comp = gmx_ingest_max_compressed(ing0);
  const uint64_t kMembers = std::min<uint64_t>(device_feed_members(), gmx_ingest_max_members(ing0));
  struct Chunk {
    size_t first, count, lo, hi;
  };
  std::vector<Chunk> chunks;
  for (size_t i = 0; i < members.size();) {
    Chunk c{i, 0, (size_t)members[i].offset, 0};
    uint64_t text = 0;
    while (i < members.size() && c.count < kMembers && text + members[i].isize <= max_text && members[i].offset + members[i].size - c.lo <= max_comp) {
      text += members[i].isize;
      c.hi = (size_t)(members[i].offset + members[i].size);
      ++c.count;
      ++i;
    }
    if (c.count == 0) return 1;
    chunks.push_back(c);
  }
  const unsigned T = feed_threads(threads);
  std::vector<gmx_bgzf_member> rel;
  auto stage = [&](size_t ci) {  // upload + inflate; the scan follows when the chunk before has been scanned
    const Chunk &c = chunks[ci];
    DeviceFeed &df = device_feed(ci % N);
    const int slot = (int)((ci / N) & 1);
    file.copy(c.lo, c.hi, df.stage[slot], T);
    rel.assign(members.begin() + (long)c.first, members.begin() + (long)(c.first + c.count));
    for (auto &m : rel) m.offset -= c.lo;
    GMX_CHECK(gmx_ingest_submit_bgzf_deferred(df.ing, slot, df.stage[slot].data(), c.hi - c.lo, rel.data(), rel.size()));
    feed_trace("chunk submitted to its device (inflate)");
    return true;
  };
  return feed_chunks_dealt(N, chunks.size(), FeedRoute::Bgzf, "chunk scanned", path, stage, on_chunk, delivered);
}

// Text slices as the dealt source (gmx_ingest_submit_text_deferred).
template <class OnChunk>
int ingest_text_file_dealt(const std::string &path, int threads, const std::vector<int> &devs, OnChunk on_chunk, uint64_t *delivered) {
  *delivered = 0;
  const size_t N = devs.size();
  uint64_t size = 0;
  if (!looks_like_plain_fastq(path, &size)) return 1;
  const ReadFile f(path);
  if (f.fd < 0) return 1;
  // (chunks of 32 MB here — scaled for nested PRGs —: every engine's ingest and its two page-locked buffers are made for the chunk size
  //  the moment the first plain file arrives — N x (1.1 GB of device memory + 256 MB page-locked) at the single-engine size of 128 MB
  //  cost a four-engine run 0.25 s before its first read was mapped, tools/cli_dealt_text.sh)
  const uint64_t chunk = std::min<uint64_t>(getenv("GMX_TEXT_CHUNK") ? device_feed_text_chunk() : device_feed_text_chunk() / 4, size);
  if (!device_feeds_ready(devs.data(), N, device_feed_text_room(chunk))) return 1;
  const size_t n_chunks = (size_t)((size + chunk - 1) / chunk);
  const unsigned T = feed_threads(threads);
  auto stage = [&](size_t ci) {
    const uint64_t lo = (uint64_t)ci * chunk;
    const size_t n = (size_t)std::min<uint64_t>(chunk, size - lo);
    DeviceFeed &df = device_feed(ci % N);
    const int slot = (int)((ci / N) & 1);
    df.stage[slot].resize(n + 64);
    if (!f.copy(lo, lo + n, df.stage[slot].data(), T)) return false;
    GMX_CHECK(gmx_ingest_submit_text_deferred(df.ing, slot, df.stage[slot].data(), n));
    feed_trace("text chunk submitted to its device");
    return true;
  };
  return feed_chunks_dealt(N, n_chunks, FeedRoute::Text, "text chunk scanned", path, stage, on_chunk, delivered);
}

// ---- the route a file takes --------------------------------------------------------------------------------------------------
// BGZF first; a file it declined with nothing delivered is tried as plain gzip (one engine: the stream's window would travel
// through the host) and, where it does not look like gzip, as plain text — each where the caller allows it. `dealt`: the chunks
// go round all of devs' engines, else to the first. *ran: the route whose return value this is.
template <class OnChunk>
int ingest_reads_file(const std::string &path, int threads, const std::vector<int> &devs, bool dealt, bool allow_gzip, bool allow_text, OnChunk on_chunk,
                      uint64_t *delivered, FeedRoute *ran) {
  *ran = FeedRoute::Bgzf;
  int rc = dealt ? ingest_bgzf_file_dealt(path, threads, devs, on_chunk, delivered) : ingest_bgzf_file(path, threads, devs[0], on_chunk, delivered);
  auto declined = [&]() { return rc == 1 && *delivered == 0; };
  if (declined() && allow_gzip && looks_like_gzip(path, nullptr)) {  // (pieces decoded side by side: DESIGN.md §11.2)
    *ran = FeedRoute::Gzip;
    return ingest_gzip_file(path, threads, devs[0], on_chunk, delivered);
  }
  if (declined() && allow_text) {  // (plain text through the same kernels minus the inflate kernel)
    *ran = FeedRoute::Text;
    rc = dealt ? ingest_text_file_dealt(path, threads, devs, on_chunk, delivered) : ingest_text_file(path, threads, devs[0], on_chunk, delivered);
  }
  return rc;
}

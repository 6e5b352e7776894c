// gmx_engine_state.h — the host side of the device half, first of five headers of the ONE translation unit gmx_engine.hip
// (included there, in this order): the engine object and what it owns — device buffers, the batch workspace, the per-read logs,
// the host feeds' slots — and the waits and the queued reset every other part uses. gmx_engine_create.h: creation (index upload,
// shared per device), destruction, the resets. gmx_engine_batch.h: one batch's launches on three streams, the grouped log's
// accounting. gmx_engine_feeds.h: the feeds of the C ABI (bytes, bit planes, 2-bit stream, planes already in HBM).
// gmx_engine_readback.h: sync, timing, coverage read-back, the block-layout switches.
#pragma once
// ===========================================================================
// engine (host side of the device half)
// ===========================================================================
#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      gmx_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
      return GMX_EHIP;                                                                     \
    }                                                                                      \
  } while (0)

// kernels timed one by one besides gmx_extend_kernel (gmx_timing::kernel_ms; include/gmx.h lists them)
enum : int { GMX_TK_SEED = 0, GMX_TK_FILTER0, GMX_TK_FILTER1, GMX_TK_SINGLE, GMX_TK_EXTEND2, GMX_TK_UNPACK, GMX_TK_N };
static_assert(GMX_TK_N <= GMX_TIMED_KERNELS, "gmx_timing::kernel_ms holds GMX_TIMED_KERNELS entries");

// A per-read log: `stride` bytes per read handed over since the last reset, appended launch by launch to one device
// buffer. Bytes from the recorded prefix on are zero (the kernels OR into zeroed words); the buffer is not an entry of
// gmx_engine::allocs: a growing one replaces it. Only reserve, clear, claim and release change d, cap and count.
struct GmxReadLog {
  const uint32_t stride;  // bytes per read
  bool on = false;
  uint32_t *d = nullptr;
  uint64_t cap = 0, count = 0;  // bytes (a multiple of 4) | reads recorded

  // the recorded prefix in bytes, to whole words: launches share the words of a log whose stride is no multiple of 4
  uint64_t used() const { return (count * stride + 3) & ~3ull; }

  // room for n_more reads (never while one of the engine's kernels is being enqueued: before the batch's first). Growth waits
  // for the launches in flight — they write the old buffer — and carries their records over.
  int reserve(uint64_t n_more) {
    const uint64_t need = (count + n_more) * stride;
    if (need <= cap) return GMX_OK;
    const uint64_t grown = (std::max<uint64_t>(need + need / 2, 1u << 20) + 3) & ~3ull;
    uint32_t *q = nullptr;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMalloc((void **)&q, grown));
    hipError_t err = hipMemset(q, 0, grown);
    if (err == hipSuccess && count) err = hipMemcpy(q, d, used(), hipMemcpyDeviceToDevice);
    if (err != hipSuccess) {
      (void)hipFree(q);
      HIP_TRY(err);
    }
    release();
    d = q;
    cap = grown;
    return GMX_OK;
  }
  // the recorded prefix back to zero — on *stream, behind what that stream holds, or at once (null) — and the count with it
  int clear(const hipStream_t *stream) {
    if (count) HIP_TRY(stream ? hipMemsetAsync(d, 0, used(), *stream) : hipMemset(d, 0, used()));
    count = 0;
    return GMX_OK;
  }
  // a launch of n reads: the index of its first read (room was made by reserve)
  uint64_t claim(uint64_t n) {
    const uint64_t base = count;
    count += n;
    return base;
  }
  void release() {
    if (d) (void)hipFree(d);
    d = nullptr;
    cap = 0;
  }
};

// The device buffers of one owner (an engine, a workspace, the shared index), each with its size: what is superseded is freed at
// once (release), the rest when the owner goes (release_all); bytes() is what gmx_engine_debug_owned_bytes adds up.
struct GmxAllocs {
  struct Buf { void *p; size_t bytes; };
  std::vector<Buf> v;

  void room(size_t n) { v.reserve(v.size() + n); }  // (the bookkeeping of the next n buffers: may throw BEFORE there is device memory to lose)
  template <class T>
  int alloc(T **p, size_t count, bool zero) {
    void *q = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    room(1);
    HIP_TRY(hipMalloc(&q, bytes));
    if (zero) {
      const hipError_t err = hipMemset(q, 0, bytes);
      if (err != hipSuccess) (void)hipFree(q);
      HIP_TRY(err);
    }
    v.push_back(Buf{q, bytes});
    *p = (T *)q;
    return GMX_OK;
  }
  void release(void *q) {
    if (!q) return;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i].p == q) {
        v[i] = v.back();
        v.pop_back();
        (void)hipFree(q);
        return;
      }
  }
  void release_all() {
    for (const Buf &b : v) (void)hipFree(b.p);
    v.clear();
  }
  uint64_t bytes() const {
    uint64_t n = 0;
    for (const Buf &b : v) n += b.bytes;
    return n;
  }
};

// A device buffer that grows with its use: `cap` elements of T are usable (gmx_engine::grow)
template <class T>
struct GmxBuf {
  T *d = nullptr;
  uint64_t cap = 0;
};

// The batch workspace: everything ensure_batch_capacity sizes for cap_reads reads per launch. One value — a growing engine builds
// a fresh one and swaps it in once all of it exists; the superseded buffers stay in `allocs` until the engine is destroyed — and
// `o` is what a launch starts from: every per-batch pointer and capacity of SearchOut (inst_cap among them), the launch fills
// in the rest (launch_batch).
struct GmxWorkspace {
  uint64_t cap_reads = 0;
  SearchOut o{};
  uint8_t *d_skip = nullptr;  // reads with a non-ACGT byte (gmx_pack_kernel writes it)
  BigOut big{};               // the large-capacity pass: one slot of pools per task it may have to take
  // grouped log: two sets of retry lists (a replay reads one and appends to the other; gmx_engine::log_retry_side)
  uint32_t *log_retry[2] = {nullptr, nullptr}, *log_retry_recs[2] = {nullptr, nullptr}, *log_retry_huge[2] = {nullptr, nullptr};
  GmxAllocs allocs;
};

// One slot of a pipelined host feed: device buffers for a chunk's payload (bytes: the reads as they came, bit planes or a 2-bit
// stream), offsets, seeds and skip flags, the byte feed's page-locked offsets and seeds (it rebases the one, and both may come from
// pageable memory), and two events: the chunk is on the device | its batch has ended. The upload of a chunk (copy stream) runs
// beside the kernels of the chunks before.
struct GmxFeedSlot {
  GmxBuf<uint8_t> payload;
  GmxBuf<uint64_t> offsets;
  GmxBuf<uint32_t> seeds;
  GmxBuf<uint8_t> skip;
  uint64_t *h_offsets = nullptr;
  uint32_t *h_seeds = nullptr;
  uint64_t h_cap = 0;  // reads the two hold
  hipEvent_t copied = nullptr, done = nullptr;
  bool busy = false;
};
enum : int { GMX_BYTE_SLOTS = 2, GMX_PACK_SLOTS = 3 };  // gmx_map_reads_host: slots [0, 2) | the packed feeds: the three behind

struct gmx_engine {
  gmx_engine_opts opts;
  GmxIndexView dview;  // device pointers
  GmxAllocs allocs;    // what the engine owns besides its workspace (until they are handed to the shared object: the index tables)
  uint64_t index_bytes = 0;
  // accumulators
  uint32_t *d_fused = nullptr, *d_limbs = nullptr;  // accumulator block (n_acc words, gmx_types.h) | 32 counter-limb words
  size_t n_fused = 0, n_acc = 0;
  // Coverage per strand (gmx_engine_record_strands): two accumulator blocks of n_acc words, forward tasks' then reverse-complement
  // tasks' (CoverAcc::rev_off = n_acc), the limbs behind both: n_fused = 2 * n_acc + 32. Off: one block, rev_off = 0.
  bool record_strands = false;
  // Per-site ambiguity counts (gmx_engine_record_site_ambiguity): 2 * n_sites words (drawn, passed per site) rounded
  // up to 64, inside the fused block between the accumulator block or blocks and the limbs — the resets, the all-reduce and the
  // peer-copy fallback carry them as they carry the second block. Off: n_tally = 0. The twin reads its owner's switch.
  bool record_site_ambiguity = false;
  size_t n_tally = 0;
  size_t tally_off() const {  // words from d_fused to them; 0: off
    const gmx_engine *w = owner ? owner : this;
    return w->record_site_ambiguity ? (w->record_strands ? 2 : 1) * n_acc : 0;
  }
  // Links between nearby sites (gmx_engine_record_links; gmx_link.h): n_links words rounded up to 64, inside the fused
  // block behind the tally — [block | (reverse block) | tally | links | limbs] — so the resets and the exchange carry them too.
  // d_link_sites: the device-only table of per-site words, built when the switch is turned on. link_span 0: off. The twin reads its
  // owner's switch, table and sizes.
  int link_span = 0;
  size_t n_links = 0;        // words of the layout (off[n_sites]); the block holds them rounded up to 64
  GmxLinkSite *d_link_sites = nullptr;
  std::vector<uint8_t> link_alleles;  // per site: A'(s) (gmx_link_alleles of its allele count), kept from the host index
  size_t links_off() const {  // words from d_fused to the link block; 0: off
    const gmx_engine *w = owner ? owner : this;
    return w->link_span ? (w->record_strands ? 2 : 1) * n_acc + w->n_tally : 0;
  }
  GmxLinks links() const {  // a kernel argument of its own (CoverAcc has no padding left); counts == nullptr: off
    const gmx_engine *w = owner ? owner : this;
    if (!w->link_span) return GmxLinks{nullptr, nullptr, 0u, 0u};
    return GmxLinks{w->d_link_sites, d_fused + links_off(), (uint32_t)w->link_span, dview.n_sites};
  }
  // The limit on a selection's candidates (gmx_engine_set_max_candidates; 0: none). Like record_strands it changes
  // only while nothing is recorded, and the twin reads its owner's: a replay or the second workspace meets the first pass's value.
  uint32_t max_candidates = 0;
  bool recorded = false;  // something may have been added to the block since it was last zeroed (launches, an exchange)
  std::vector<uint32_t> phys_allele, phys_pb, phys_grouped;  // logical slot -> slot of the block (gmx_coverage_fetch)
  std::vector<uint32_t> hit_fix;                             // hit counters and the logical slots they count for
  unsigned long long *d_stats = nullptr;  // with d_log_cursor behind the coverage block: one memset resets all of it
  uint32_t *d_error = nullptr;
  uint32_t *d_log = nullptr, *d_log_cursor = nullptr;
  uint32_t log_cap = 0;
  uint32_t n_allele = 0, n_pb = 0, n_grouped = 0;
  GmxWorkspace ws;                // the batch workspace (ensure_batch_capacity: sized by the largest launch so far)
  GmxBuf<uint2> packed;           // the bit planes of a launch whose reads arrive as bytes or as a 2-bit stream (pairs)
  uint32_t *d_counters = nullptr; // per-batch queue counters (SearchOut::counters): the resets and log_state_enqueue read them too
  bool cover_jump = false;  // gmx_cover_jump_kernel + gmx_cover_single_rest_kernel instead of gmx_cover_single_kernel<false>
  bool seed_cursor = false;  // the index has many multi-state k-mer entries: kernels instantiated with the seed cursor
  uint32_t *d_scratch_big = nullptr;  // the scratch of the coverage instance with the largest one (gmx_cover_kernel<CoverEnvBig, 1>)
  uint32_t cover_big_lanes = 0;
  bool coop = true;  // GMX_NO_COOP=1 in the environment: serial coverage instances only (A/B runs)
  uint32_t *d_heap = nullptr;      // the last tier's memory (gmx_tail_stage)
  uint64_t heap_words = 0;
  bool log_sites = false;          // the index has sites with more than 8 alleles
  // grouped log: drained into `log_counts` (records with counts) whenever the device log may run full, and at fetch time
  // key = [site_index, ids...]; value = the records of forward and of reverse-complement tasks (GMX_LOG_REVERSE: the second
  // is zero unless the engine records strands)
  std::map<std::vector<uint32_t>, std::array<uint64_t, 2>> log_counts;
  // Exact accounting (round 3): after every batch of an engine whose index uses the log, the log cursor and the lengths
  // of the three retry lists are copied to page-locked words; before the next batch (and before any reader of the
  // coverage) log_settle() looks at them: entries that found the log full are redone after a drain (launch_log_replay),
  // and the log is drained once it is half full. No assumed bound on what a read appends.
  uint32_t *h_log_state = nullptr;     // [cursor, retry entries, retry records, retry last-tier tasks]
  hipEvent_t ev_log_state = nullptr;
  bool log_state_pending = false;
  int log_retry_side = 0;              // which of the workspace's two sets of retry lists the kernels append to
  BatchView last_b{};
  SearchOut last_o{};
  CoverAcc last_acc{};
  size_t last_big_lds = 0;
  uint64_t log_replays = 0, log_replayed_entries = 0;  // statistics (tests)
  uint64_t log_known = 0;          // log words in use after the last drain / look ...
  uint64_t log_reads_since = 0;    // (unused since round 3: the fill is read back after every batch)
  // gmx_engine_reset_async leaves its memset pending: the next batch's pack kernel zeroes the block when it is launched
  // on the same stream (one command and one dependent-launch gap less per job); every other reader of the accumulators
  // issues the memset first (flush_reset)
  bool reset_pending = false;
  hipStream_t reset_stream = nullptr;
  hipStream_t side2_stream = nullptr;
  hipEvent_t ev_fork2 = nullptr, ev_side1 = nullptr, ev_filter = nullptr;
  hipStream_t side_stream = nullptr;  // large-capacity search + its coverage run beside filter/cover
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_wait = nullptr;  // blocking event of gmx_quiesce
  struct GmxDeviceIndex *shared_index = nullptr;  // the device copy of the index tables, shared with the other engines of this index on this device
  uint32_t filter_lds_words = 0;  // > 0: the k-mer presence bitmap fits LDS (gmx_filter_lds_kernel)
  const uint32_t *d_kmer_planar = nullptr;  // that bitmap indexed by planar k-mer code (all_kmers_present_planar)
  const uint32_t *d_absent = nullptr;       // the k-mers that do NOT occur, when they are few (gmx_filter_absent_kernel)
  uint32_t n_absent = 0;
  bool use_absent = false;
  uint32_t n_cus = 256;
  uint32_t probe_iters = GMX_PROBE_ITERS;  // wave-loop iterations before the probe kernel parks what is left
  uint32_t extend_cap = 0;      // iterations of the LAST pass after which a task goes to the large-capacity route (0: runs to the end)
  uint32_t extend_budget = 8;   // wave-loop iterations of the extend kernel before a lane with work left is parked for the second pass
  bool seeds_in_place = false;  // gmx_engine_seeds_in_place
  // A second batch in flight (round 6). Every batch ends with a tail of few-lane kernels — on a nested PRG ~2 ms of a few straggler
  // tasks on a handful of CUs — during which the GPU is all but idle. The TWIN is a second workspace with streams of its own that
  // shares this engine's index and ACCUMULATORS (coverage is atomic adds: two batches may record side by side): the host feeds hand
  // consecutive launches to engine and twin in turn, so launch i + 1's full-GPU kernels run beside launch i's tail. Measured with
  // two engines per device in round 5 (tools/exp/engines_in_flight.py): configs[2] 388 -> 499 M reads/s at 1 M reads per launch,
  // configs[3] + 11 %, configs[1] +- 0 — so the twin exists for nested PRGs and indexes of 2 GB and more (GMX_TWIN=0 / 1 forces),
  // never for an index whose sites use the grouped log (its replay is per batch).
  gmx_engine *twin = nullptr;
  gmx_engine *owner = nullptr;  // (of a twin: the engine it belongs to)
  bool is_twin = false, twin_off = false;
  // The per-read logs, in the ENGINE's buffers whichever workspace runs the launch — a launch is given its first read's index
  // when it is enqueued. Outcomes (gmx_engine_record_outcomes; SearchOut::outcomes): one byte per read. Positions
  // (gmx_engine_record_positions; SearchOut::positions): 16 bytes per read — [pos, n] of the forward task, [pos, n] of
  // the reverse-complement one.
  GmxReadLog outcomes{1}, positions{16};
  uint64_t reset_epoch = 0;  // resets so far (gmx_group: are its ledgers of ranges still about these buffers?)
  hipStream_t main_stream = nullptr;  // the twin's main chain (the engine's own: the NULL stream, or the caller's)
  uint32_t twin_toggle = 0;
  hipEvent_t ev_zeroed = nullptr, ev_twin_done = nullptr;  // a queued reset has executed | the twin's last batch has ended
  uint64_t zero_epoch = 0, seen_zero_epoch = 0;
  bool twin_in_flight = false;   // the twin has launched since the last join
  bool last_on_twin = false;     // the last launch went to the twin (gmx_engine_queue_counts reads that workspace's counters)
  uint32_t extend_passes = 1;   // launches over the stragglers (<= GMX_EXTRA_PASSES); all but the last with a budget of their own
  uint32_t extend_budget2[GMX_EXTRA_PASSES] = {24, 96, 0};
                                // (GMX_EXTEND_BUDGET in the environment; 0 = one pass)
  // test hook (gmx_engine_debug_keep_states, gmx_debug_final_states): the last batch's per-task search results stay readable
  bool keep_states = false;
  uint64_t keep_reads = 0;            // reads of that batch
  std::vector<uint32_t> debug_isa;    // inverse suffix array (text position -> SA index), fetched on first use
  uint32_t fuse = 1;  // fused transitions in the extend kernel's wave loop (GMX_NO_FUSE=1 in the environment: off, for A/B runs)
  // host staging of the _host entry point's serial path (one batch in flight)
  GmxBuf<uint8_t> stage_reads;
  GmxBuf<uint64_t> stage_offsets;
  GmxBuf<uint32_t> stage_seeds;
  // the pipelined host feeds: gmx_map_reads_host takes its two slots in turn from the first of every call, the packed feeds go
  // round their three from call to call (pack_next); the uploads run on a copy stream
  GmxFeedSlot slots[GMX_BYTE_SLOTS + GMX_PACK_SLOTS];
  uint32_t pack_next = 0;
  hipStream_t copy_stream = nullptr;
  hipStream_t copy_stream2 = nullptr;  // the packed feeds' uploads alternate between the two (gmx_map_reads_packed_host / _2bit_host)
  uint32_t copy_toggle = 0;
  hipStream_t last_stream = nullptr;
  template <class T>
  int alloc(T **p, size_t count, bool zero) { return allocs.alloc(p, count, zero); }
  // releases a device buffer obtained from alloc() before the engine is destroyed (a superseded or temporary one)
  void release(void *q) { allocs.release(q); }
  // The ONE way a device buffer of the engine grows: nothing to do while `need` elements fit; else one of `grown` usable elements
  // (the caller's growth rule: its slack and headroom) + `tail` more takes its place.
  // in_flight: work already enqueued may still read the old buffer (the bit planes and the serial staging at launch time) — it
  // stays in `allocs` until the engine is destroyed, and a failure leaves the buffer as it was. Otherwise (a slot's buffers, idle
  // once the slot is acquired) the superseded buffer is freed first, and a failure leaves the buffer empty (cap 0), never dangling.
  template <class T>
  int grow(GmxBuf<T> &b, uint64_t need, uint64_t grown, uint64_t tail, bool in_flight) {
    if (need <= b.cap) return GMX_OK;
    T *q = nullptr;
    if (!in_flight) {
      allocs.room(1);
      allocs.release(b.d);
      b.d = nullptr;
      b.cap = 0;
    }
    const int rc = allocs.alloc(&q, grown + tail, false);
    if (rc) return rc;
    b.d = q;
    b.cap = grown;
    return GMX_OK;
  }
  // optional HIP-event timing of the kernels (bench.py roofline leg)
  bool timing = false;
  struct EvTriple { hipEvent_t s, a, b, c; uint64_t reads; hipEvent_t k[GMX_TIMED_KERNELS][2]; uint32_t timed; };
  std::vector<EvTriple> pending;
  double search_ms = 0, cover_ms = 0;
  uint64_t search_launches = 0, cover_launches = 0, timed_reads = 0;
  double kernel_ms[GMX_TIMED_KERNELS] = {0};        // gmx_timing::kernel_ms (GMX_TK_*)
  uint64_t kernel_launches[GMX_TIMED_KERNELS] = {0};

  template <class T, class A>
  int upload(const T **dst, const std::vector<T, A> &src) {
    T *q = nullptr;
    int rc = alloc(&q, src.size(), false);
    if (rc) return rc;
    if (!src.empty()) HIP_TRY(hipMemcpy(q, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    index_bytes += src.size() * sizeof(T);
    *dst = q;
    return GMX_OK;
  }
  int upload(const uint32_t **dst, const gmx::WordBuf &src) {
    uint32_t *q = nullptr;
    int rc = alloc(&q, src.size(), false);
    if (rc) return rc;
    const size_t piece = (size_t)1 << 28;  // (pageable memory, tens of GB at whole-genome scale: 1 GB per staged copy)
    for (size_t at = 0; at < src.size(); at += piece)
      HIP_TRY(hipMemcpy(q + at, src.data() + at, std::min(piece, src.size() - at) * sizeof(uint32_t), hipMemcpyHostToDevice));
    index_bytes += src.size() * sizeof(uint32_t);
    *dst = q;
    return GMX_OK;
  }
};

// Host-side wait for an event that costs no core: query, nap, query. hipEventSynchronize — also on an event created with
// hipEventBlockingSync — kept the calling thread AND a thread of the runtime at 100 % of a core each on the GPU boxes
// (tools/exp/host_call_cost.py: 1500 back-to-back calls, 1.03 s of wall time, 1.03 s of CPU in each of the two threads), so a
// feeder that runs ahead of its GPU cost two cores: eight of them, sixteen — the whole container. The nap (50 us) is far
// below a batch (0.4-3 ms) and three batches are in flight per engine, so the GPU never waits for the host's wake-up.
// GMX_WAIT_SPIN=1: hipEventSynchronize as before (A/B runs).
static hipError_t gmx_event_wait(hipEvent_t ev) {
  static const bool spin = getenv("GMX_WAIT_SPIN") != nullptr;
  if (spin) return hipEventSynchronize(ev);
  // (the first 60 us by querying alone: an event about to complete — the end of a job, the last of several streams — is
  //  not paid for with a nap's wake-up latency; a feeder ahead of its GPU waits ~0.5 ms per batch and naps through it)
  const auto t0 = std::chrono::steady_clock::now();
  for (bool napping = false;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q != hipErrorNotReady) return q;
    (void)hipGetLastError();  // (hipErrorNotReady is sticky for hipGetLastError)
    if (!napping) {
      napping = std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(60);
      continue;
    }
    struct timespec ts = {0, 50 * 1000};
    nanosleep(&ts, nullptr);
  }
}

// Wait for the engine's own streams WITHOUT spinning: a blocking event per stream (the thread sleeps until the interrupt).
// hipStreamSynchronize / hipDeviceSynchronize poll — one core per waiting thread; a node's eight feeder threads, each ahead
// of its GPU, cost eight cores that way (profiles/round4/feed_x8.txt: 2.5 ns of host CPU per read, 27 cores' worth at
// 8 x 1.34 G reads/s). The callers still issue their hipDeviceSynchronize afterwards: it then returns at once.
static int gmx_quiesce(gmx_engine *e) {
  if (!e->ev_wait) HIP_TRY(hipEventCreateWithFlags(&e->ev_wait, hipEventDisableTiming | hipEventBlockingSync));
  hipStream_t streams[5] = {e->last_stream, e->copy_stream, e->side_stream, e->side2_stream, e->copy_stream2};
  for (int i = 0; i < 5; ++i) {
    if (i > 0 && !streams[i]) continue;  // ([0]: the null stream counts)
    bool seen = false;
    for (int j = 0; j < i; ++j) seen = seen || streams[j] == streams[i];
    if (seen) continue;
    HIP_TRY(hipEventRecord(e->ev_wait, streams[i]));
    HIP_TRY(gmx_event_wait(e->ev_wait));
  }
  return GMX_OK;
}

// the accumulators have been zeroed by work on `stream` (a queued reset): the twin's next batch must come behind it
static int note_zeroed(gmx_engine *e, hipStream_t stream) {
  if (!e->twin) return GMX_OK;
  if (!e->ev_zeroed) HIP_TRY(hipEventCreateWithFlags(&e->ev_zeroed, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(e->ev_zeroed, stream));
  ++e->zero_epoch;
  return GMX_OK;
}
// `stream` waits for the twin's last batch (its main stream joins its side streams at the end of every batch)
static int twin_join(gmx_engine *e, hipStream_t stream) {
  gmx_engine *tw = e->twin;
  if (!tw || !e->twin_in_flight) return GMX_OK;
  if (!e->ev_twin_done) HIP_TRY(hipEventCreateWithFlags(&e->ev_twin_done, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(e->ev_twin_done, tw->main_stream));
  HIP_TRY(hipStreamWaitEvent(stream, e->ev_twin_done, 0));
  return GMX_OK;
}
static int flush_reset(gmx_engine *e) {
  if (!e->reset_pending) return GMX_OK;
  e->reset_pending = false;
  HIP_TRY(hipMemsetAsync(e->d_fused, 0, (e->n_fused + 32) * 4, e->reset_stream));
  return note_zeroed(e, e->reset_stream);
}

// gmx_engine_feeds.h — part of gmx_engine.hip's translation unit (gmx_engine_state.h lists the parts): the feeds of the C ABI. Reads
// in device memory, reads in host memory as bytes (serial, or pipelined through two slots), as bit planes or a 2-bit stream
// (three slots), planes already in HBM; which workspace a launch takes (pick_target); the reserve calls; page-locked host memory.
#pragma once
// Is [p, p + bytes) page-locked memory the runtime can DMA from asynchronously (gmx_host_alloc, hipHostMalloc, registered)?
static bool gmx_is_pinned(const void *p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// ---- the slot ring of the pipelined host feeds (GmxFeedSlot) --------------------------------------------------------------
// acquire: the chunk that used the slot a round ago has ended (a wait that costs no core: gmx_event_wait); the events on first use
static int slot_acquire(GmxFeedSlot &sl) {
  if (sl.busy) {
    HIP_TRY(gmx_event_wait(sl.done));
    sl.busy = false;
  }
  if (!sl.copied) HIP_TRY(hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming | hipEventBlockingSync));
  if (!sl.done) HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming | hipEventBlockingSync));
  return GMX_OK;
}
// What a chunk needs of a slot and the capacities its feed's growth rule gives: payload bytes (+ `tail` bytes behind them) | reads
struct SlotNeed {
  uint64_t bytes, bytes_grown, tail, reads, reads_grown;
};
// grow (the slot is idle: its superseded buffers go at once). The byte feed's slots have page-locked offsets and seeds and no skip flags.
static int slot_grow(gmx_engine *e, GmxFeedSlot &sl, const SlotNeed &n, bool byte_feed) {
  int rc;
  if ((rc = e->grow(sl.payload, n.bytes, n.bytes_grown, n.tail, false)) || (rc = e->grow(sl.offsets, n.reads, n.reads_grown, 1, false)) ||
      (rc = e->grow(sl.seeds, n.reads, n.reads_grown, 0, false)))
    return rc;
  if (!byte_feed) return e->grow(sl.skip, n.reads, n.reads_grown, 0, false);
  // (page-locked host memory is no entry of `allocs`, so it does not go through grow(); h_cap stays 0 until both buffers exist)
  if (n.reads <= sl.h_cap) return GMX_OK;
  if (sl.h_offsets) (void)hipHostFree(sl.h_offsets);
  if (sl.h_seeds) (void)hipHostFree(sl.h_seeds);
  sl.h_offsets = nullptr;
  sl.h_seeds = nullptr;
  sl.h_cap = 0;
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl.h_offsets), (n.reads_grown + 1) * sizeof(uint64_t), hipHostMallocDefault));
  HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl.h_seeds), n.reads_grown * sizeof(uint32_t), hipHostMallocDefault));
  sl.h_cap = n.reads_grown;
  return GMX_OK;
}
// the chunk's copies are queued on `copy`: the batch on `launch` comes behind them
static int slot_copied(GmxFeedSlot &sl, hipStream_t copy, hipStream_t launch) {
  HIP_TRY(hipEventRecord(sl.copied, copy));
  HIP_TRY(hipStreamWaitEvent(launch, sl.copied, 0));
  return GMX_OK;
}
// the batch is queued on `launch`: the slot is its until it has ended
static int slot_done(GmxFeedSlot &sl, hipStream_t launch) {
  HIP_TRY(hipEventRecord(sl.done, launch));
  sl.busy = true;
  return GMX_OK;
}

// The frame of a pipelined host feed. What of the caller's memory the runtime cannot DMA from is registered for the duration of the
// call; the loop runs; the epilogue ALWAYS runs — an error or an exception (host memory) must not skip it: memory is registered,
// copies are in flight. It waits for the uploads, which read the caller's buffers, when the call failed or registered memory; a
// failed call also waits for the device and leaves the ring idle. `drain`: the feed does all of that whatever happened.
struct HostSpan {
  const void *p;
  uint64_t bytes;
};
template <size_t N, class Loop>
static int feed_frame(gmx_engine *e, const char *who, const HostSpan (&spans)[N], GmxFeedSlot *ring, int n_slots, bool drain, Loop loop) {
  bool registered[N], all_pinned = true;
  for (size_t i = 0; i < N; ++i) {
    registered[i] = false;
    if (!spans[i].p || gmx_is_pinned(spans[i].p)) continue;
    registered[i] = hipHostRegister(const_cast<void *>(spans[i].p), spans[i].bytes, hipHostRegisterDefault) == hipSuccess;
    (void)hipGetLastError();
    all_pinned = false;
  }
  int rc;
  try {
    rc = loop();
  } catch (...) {
    rc = gmx_guard_catch(who);
  }
  if (drain || rc != GMX_OK || !all_pinned) {
    (void)hipStreamSynchronize(e->copy_stream);
    if (e->copy_stream2) (void)hipStreamSynchronize(e->copy_stream2);
    if (drain || rc != GMX_OK) {
      (void)hipDeviceSynchronize();
      for (int i = 0; i < n_slots; ++i) ring[i].busy = false;
    }
  }
  for (size_t i = 0; i < N; ++i)
    if (registered[i]) (void)hipHostUnregister(const_cast<void *>(spans[i].p));
  (void)hipGetLastError();
  return rc;
}

extern "C" {

int gmx_map_reads_device(gmx_engine *e, const uint8_t *d_reads, const uint64_t *d_offsets, const uint32_t *d_seeds,
                         uint64_t n_reads, uint64_t total_bases, void *hip_stream) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  hipStream_t stream = (hipStream_t)hip_stream;
  uint64_t done = 0;
  while (done < n_reads) {
    uint64_t n = std::min<uint64_t>(e->opts.max_batch_reads, n_reads - done);
    BatchInput in;
    in.d_reads = d_reads;
    in.d_offsets = d_offsets + done;
    in.d_seeds = d_seeds + done;
    in.n_reads = n;
    in.total_bases = total_bases;
    int rc = launch_batch(e, in, stream);
    if (rc) return rc;
    done += n;
  }
  // An index with log sites: a batch that found the grouped log full is replayed from ITS inputs (read lengths, seeds), and
  // the caller may reuse its device buffers in stream order after this call: settle now (waits for the batch; engines
  // without log sites — every dense-count index — stay asynchronous).
  if (e->log_sites) return log_settle(e);
  return GMX_OK;
} GMX_GUARD_INT("gmx_map_reads_device")

// Large calls: chunks of <= 1 M reads through two staging slots; the upload of a chunk (copy stream, from the caller's
// buffer registered with the runtime for the duration of the call) runs beside the kernels of the one before. The feed drains:
// when it returns nothing in flight reads the caller's buffer and the slots are idle.
static int map_reads_host_pipelined(gmx_engine *e, const uint8_t *reads, const uint64_t *offsets, const uint32_t *seeds,
                                    uint64_t n_reads, uint64_t chunk) {
  if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  const HostSpan spans[1] = {{reads + offsets[0], offsets[n_reads] - offsets[0]}};
  const int rc = feed_frame(e, "gmx_map_reads_host", spans, e->slots, GMX_BYTE_SLOTS, true, [&]() -> int {
    uint64_t done = 0;
    for (uint32_t i = 0; done < n_reads; ++i) {
      GmxFeedSlot &sl = e->slots[i % GMX_BYTE_SLOTS];
      const uint64_t n = std::min<uint64_t>(chunk, n_reads - done);
      const uint64_t b0 = offsets[done], bases = offsets[done + n] - b0;
      int lrc = slot_acquire(sl);  // the chunk that used this slot two rounds ago
      if (lrc || (lrc = slot_grow(e, sl, SlotNeed{bases, std::max<uint64_t>(bases + bases / 8, 1 << 16), 16, n, std::max<uint64_t>(n, 1024)}, true)))
        return lrc;
      for (uint64_t j = 0; j <= n; ++j) sl.h_offsets[j] = offsets[done + j] - b0;
      memcpy(sl.h_seeds, seeds + done, n * sizeof(uint32_t));
      HIP_TRY(hipMemcpyAsync(sl.payload.d, reads + b0, bases, hipMemcpyHostToDevice, e->copy_stream));
      HIP_TRY(hipMemcpyAsync(sl.offsets.d, sl.h_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->copy_stream));
      HIP_TRY(hipMemcpyAsync(sl.seeds.d, sl.h_seeds, n * sizeof(uint32_t), hipMemcpyHostToDevice, e->copy_stream));
      if ((lrc = slot_copied(sl, e->copy_stream, nullptr))) return lrc;
      BatchInput in;
      in.d_reads = sl.payload.d;
      in.d_offsets = sl.offsets.d;
      in.d_seeds = sl.seeds.d;
      in.n_reads = n;
      in.total_bases = bases;
      if ((lrc = launch_batch(e, in, nullptr)) || (lrc = slot_done(sl, nullptr))) return lrc;
      done += n;
    }
    return GMX_OK;
  });
  return rc ? rc : gmx_engine_sync(e);
}

static uint64_t gmx_feed_chunk(const gmx_engine *e);  // reads per launch of the host feeds (below)
int gmx_map_reads_host(gmx_engine *e, const uint8_t *reads, const uint64_t *offsets, const uint32_t *seeds,
                       uint64_t n_reads) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  if (n_reads == 0) return GMX_OK;
  HIP_TRY(hipSetDevice(e->opts.device));
  {
    const uint64_t chunk = gmx_feed_chunk(e);
    if (n_reads > chunk && !getenv("GMX_HOST_SERIAL")) return map_reads_host_pipelined(e, reads, offsets, seeds, n_reads, chunk);
  }
  uint64_t done = 0;
  while (done < n_reads) {
    uint64_t n = std::min<uint64_t>(e->opts.max_batch_reads, n_reads - done);
    uint64_t b0 = offsets[done], b1 = offsets[done + n];
    uint64_t bases = b1 - b0;
    // (in flight: a batch of an earlier call that failed may still read the staging; within a call each ends before the next)
    const uint64_t cr = std::max<uint64_t>(n, 1024);
    int rc = e->grow(e->stage_reads, bases, std::max<uint64_t>(bases, 1 << 16), 16, true);
    if (rc || (rc = e->grow(e->stage_offsets, n, cr, 1, true)) || (rc = e->grow(e->stage_seeds, n, cr, 0, true))) return rc;
    std::vector<uint64_t> rel(n + 1);
    for (uint64_t i = 0; i <= n; ++i) rel[i] = offsets[done + i] - b0;
    HIP_TRY(hipMemcpy(e->stage_reads.d, reads + b0, bases, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->stage_offsets.d, rel.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->stage_seeds.d, seeds + done, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    BatchInput in;
    in.d_reads = e->stage_reads.d;
    in.d_offsets = e->stage_offsets.d;
    in.d_seeds = e->stage_seeds.d;
    in.n_reads = n;
    in.total_bases = bases;
    if ((rc = launch_batch(e, in, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));  // staging buffers are reused by the next batch
    if (e->log_sites && (rc = log_settle(e))) return rc;  // ... and a replay of this batch reads them: before they are overwritten
    done += n;
  }
  return gmx_engine_sync(e);
} GMX_GUARD_INT("gmx_map_reads_host")

// Which workspace and main stream the next launch of a host feed takes: the engine's own (NULL stream) and its twin's in turn
// (gmx_engine::twin). The launch that carries a queued reset goes to the engine itself (its first kernel zeroes the accumulators);
// the twin's next launch waits for that kernel.
struct BatchTarget {
  gmx_engine *eng;
  hipStream_t stream;
};
static int pick_target(gmx_engine *e, BatchTarget *out) {
  out->eng = e;
  out->stream = nullptr;
  e->last_on_twin = false;
  gmx_engine *tw = e->twin;
  if (!tw || e->twin_off || e->keep_states) return GMX_OK;
  if (e->reset_pending) {
    e->twin_toggle = 1;
    return GMX_OK;
  }
  if ((e->twin_toggle++ & 1u) == 0) return GMX_OK;
  if (tw->seen_zero_epoch != e->zero_epoch) {
    HIP_TRY(hipStreamWaitEvent(tw->main_stream, e->ev_zeroed, 0));
    tw->seen_zero_epoch = e->zero_epoch;
  }
  tw->timing = e->timing;
  out->eng = tw;
  out->stream = tw->main_stream;
  e->twin_in_flight = true;
  e->last_on_twin = true;
  return GMX_OK;
}

// planes: the bit planes (twobit = false) or the 2-bit stream as 32-bit words (twobit = true; gmx_map_reads_2bit_host). Three slots
// in turn; a chunk goes up straight from the caller's buffers, and the call returns with uploads and batches in flight unless it
// failed or had to register memory.
static int map_reads_packed_impl(gmx_engine *e, const uint64_t *planes, bool twobit, const uint64_t *offsets, uint32_t uniform_len,
                                 const uint32_t *seeds, const uint8_t *skip, uint64_t n_reads) {
  if (!e || !planes || !seeds || (!offsets && !uniform_len)) {
    gmx_set_error("gmx_map_reads_packed_host / gmx_map_reads_2bit_host: null argument (offsets may be null only with uniform_len)");
    return GMX_EINVAL;
  }
  if (n_reads == 0) return GMX_OK;
  HIP_TRY(hipSetDevice(e->opts.device));
  if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  static const bool two_copy_streams = getenv("GMX_TWO_COPY_STREAMS") != nullptr;
  if (two_copy_streams && !e->copy_stream2) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream2, hipStreamNonBlocking));
  const uint32_t ppr = (uniform_len + 31u) / 32u;
  auto base_at = [&](uint64_t r) -> uint64_t { return uniform_len ? r * uniform_len : offsets[r] - offsets[0]; };
  auto pair_at = [&](uint64_t r) -> uint64_t {  // 8-byte units from the call's first read to read r (gmx.h: layout of `planes`;
    if (twobit) return (base_at(r) + 31) >> 5;  //  a 2-bit stream: 32 bases per unit, rounded up)
    return uniform_len ? r * ppr : ((offsets[r] >> 5) - (offsets[0] >> 5)) + r;
  };
  const uint64_t chunk = gmx_feed_chunk(e);
  GmxFeedSlot *ring = e->slots + GMX_BYTE_SLOTS;
  const HostSpan spans[4] = {{planes, pair_at(n_reads) * 8}, {offsets, (n_reads + 1) * 8}, {seeds, n_reads * 4}, {skip, n_reads}};
  return feed_frame(e, twobit ? "gmx_map_reads_2bit_host" : "gmx_map_reads_packed_host", spans, ring, GMX_PACK_SLOTS, false, [&]() -> int {
    // seeds in place (gmx_engine_seeds_in_place): the kernels read the few seeds they need — a read draws only when it has
    // several equally good mapping classes — from the caller's page-locked buffer over PCIe; nothing is uploaded
    const uint32_t *d_seeds_host = nullptr;
    if (e->seeds_in_place && gmx_is_pinned(seeds)) {
      void *dp = nullptr;
      if (hipHostGetDevicePointer(&dp, const_cast<uint32_t *>(seeds), 0) == hipSuccess && dp) d_seeds_host = static_cast<const uint32_t *>(dp);
      else (void)hipGetLastError();
    }
    for (uint64_t done = 0; done < n_reads;) {
      GmxFeedSlot &sl = ring[e->pack_next];
      e->pack_next = (e->pack_next + 1) % GMX_PACK_SLOTS;
      const uint64_t n = std::min<uint64_t>(chunk, n_reads - done);
      uint64_t p0 = pair_at(done), pairs = pair_at(done + n) - p0;
      uint32_t twobit_base0 = 0;
      if (twobit) {  // the chunk's bases from the 8-byte unit holding its first one
        const uint64_t b0 = base_at(done), b1 = base_at(done + n);
        p0 = b0 >> 5;
        pairs = ((b1 + 31) >> 5) - p0;
        twobit_base0 = (uint32_t)(b0 & 31u);
      }
      int rc = slot_acquire(sl);  // the batch that used this slot three chunks ago
      // (+ 16 pairs of slack: the kernels fetch whole 16-byte pieces and one pair ahead)
      if (rc || (rc = slot_grow(e, sl, SlotNeed{(pairs + 16) * 8, (pairs + pairs / 8 + 64) * 8, 0, n, std::max<uint64_t>(n, 1024)}, false))) return rc;
      // One copy stream. (Round 5: the box's link carries 56-57 GB/s with nothing beside it, tools/exp/h2d_rate.py, this loop 51; with
      // consecutive batches' uploads alternating between TWO streams — a copy queued behind the one in flight — the median job is 2.5 %
      // faster, 1.395 against 1.365 G reads/s, but one job in five is 20-40 % slower — two copies share the link and both batches' kernels
      // start late — where one stream's jobs lie within 0.5 % of each other. GMX_TWO_COPY_STREAMS=1 selects it. Three and four streams:
      // worse. ONE batch's planes split over two streams reached 31-37 GB/s, and a kernel pulling the stream out of the caller's
      // page-locked memory itself 34 GB/s — both measured in round 3 and removed.)
      const hipStream_t cs = two_copy_streams && ((e->copy_toggle++) & 1u) ? e->copy_stream2 : e->copy_stream;
      HIP_TRY(hipMemcpyAsync(sl.payload.d, planes + p0, pairs * 8, hipMemcpyHostToDevice, cs));
      if (!uniform_len) HIP_TRY(hipMemcpyAsync(sl.offsets.d, offsets + done, (n + 1) * 8, hipMemcpyHostToDevice, cs));
      if (!d_seeds_host) HIP_TRY(hipMemcpyAsync(sl.seeds.d, seeds + done, n * 4, hipMemcpyHostToDevice, cs));
      if (skip) HIP_TRY(hipMemcpyAsync(sl.skip.d, skip + done, n, hipMemcpyHostToDevice, cs));
      BatchTarget tg;
      if ((rc = pick_target(e, &tg)) || (rc = slot_copied(sl, cs, tg.stream))) return rc;
      BatchInput in;
      in.d_offsets = uniform_len ? nullptr : sl.offsets.d;
      in.d_seeds = d_seeds_host ? d_seeds_host + done : sl.seeds.d;
      in.d_planes = twobit ? nullptr : reinterpret_cast<const uint2 *>(sl.payload.d);
      in.d_twobit = twobit ? reinterpret_cast<const uint32_t *>(sl.payload.d) : nullptr;
      in.twobit_base0 = twobit_base0;
      in.d_skip = skip ? sl.skip.d : nullptr;
      in.uniform_len = uniform_len;
      in.n_reads = n;
      in.total_bases = uniform_len ? n * (uint64_t)uniform_len : offsets[done + n] - offsets[done];
      if ((rc = launch_batch(tg.eng, in, tg.stream)) || (rc = slot_done(sl, tg.stream))) return rc;
      done += n;
    }
    return GMX_OK;
  });
}

int gmx_map_reads_packed_host(gmx_engine *e, const uint64_t *planes, const uint64_t *offsets, uint32_t uniform_len,
                              const uint32_t *seeds, const uint8_t *skip, uint64_t n_reads) try {
  return map_reads_packed_impl(e, planes, false, offsets, uniform_len, seeds, skip, n_reads);
} GMX_GUARD_INT("gmx_map_reads_packed_host")

// Reads per launch of the host / device-plane feeds: the whole call, up to max_batch_reads (4 M). Every batch ends with a tail
// of few-lane kernels — on a NESTED PRG with ~2 ms of a few straggler tasks (reads inside MSA regions: hundreds of dependent
// general iterations each) whatever its size —, and the tail is paid per launch (round 5, tools/exp/engines_in_flight.py,
// kernel pipeline): configs[2] maps 138 M reads/s in launches of 250 k reads, 388 M at 1 M, 640 M at 4 M; configs[3] 914 M ->
// 1 173 M, configs[4] 350 -> 412 M, configs[1] 2.30 -> 2.63 G from 1 M to 4 M. (Until round 5 a launch took at most 2^20 reads;
// a call's first upload is now up to four times as long, the uploads behind it still hide behind the kernels.)
static uint64_t gmx_feed_chunk(const gmx_engine *e) {
  static const char *env = getenv("GMX_FEED_CHUNK");
  if (env) return std::max<uint64_t>(1, std::min<uint64_t>(e->opts.max_batch_reads, strtoull(env, nullptr, 10)));
  return e->opts.max_batch_reads;
}

// bit planes already in HBM (gmx_ingest_*): nothing to upload; seeds in device memory, or page-locked and read in place
int gmx_map_reads_packed_device(gmx_engine *e, const uint64_t *d_planes, const uint64_t *d_offsets, uint32_t uniform_len,
                                const uint32_t *seeds, const uint8_t *d_skip, uint64_t n_reads) try {
  if (!e || !d_planes || !seeds || (!d_offsets && !uniform_len)) {
    gmx_set_error("gmx_map_reads_packed_device: null argument (d_offsets may be null only with uniform_len)");
    return GMX_EINVAL;
  }
  if (n_reads == 0) return GMX_OK;
  HIP_TRY(hipSetDevice(e->opts.device));
  const uint32_t *d_seeds = seeds;
  if (gmx_is_pinned(seeds)) {
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<uint32_t *>(seeds), 0) != hipSuccess || !dp) {
      (void)hipGetLastError();
      gmx_set_error("gmx_map_reads_packed_device: the page-locked seeds have no device address");
      return GMX_EHIP;
    }
    d_seeds = static_cast<const uint32_t *>(dp);
  }
  const uint64_t chunk = gmx_feed_chunk(e);
  if (!uniform_len && n_reads > chunk) {
    gmx_set_error("gmx_map_reads_packed_device: with d_offsets a call takes at most 2^20 reads (and at most max_batch_reads)");
    return GMX_EINVAL;
  }
  const uint64_t ppr = (uniform_len + 31u) / 32u;
  for (uint64_t done = 0; done < n_reads;) {
    const uint64_t n = std::min<uint64_t>(chunk, n_reads - done);
    BatchInput in;
    in.d_planes = reinterpret_cast<const uint2 *>(d_planes + done * ppr);
    in.d_offsets = uniform_len ? nullptr : d_offsets;
    in.d_seeds = d_seeds + done;
    in.d_skip = d_skip ? d_skip + done : nullptr;
    in.uniform_len = uniform_len;
    in.n_reads = n;
    in.total_bases = uniform_len ? n * (uint64_t)uniform_len : 0;  // (sizes the pack buffer of byte input only)
    BatchTarget tg;
    int rc = pick_target(e, &tg);
    if (rc) return rc;
    // (the planes were written by work on the NULL stream or on streams the caller has ordered before it — gmx_ingest_wait has
    //  returned —: the twin's stream needs no extra wait for them)
    if ((rc = launch_batch(tg.eng, in, tg.stream))) return rc;
    done += n;
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_map_reads_packed_device")

int gmx_map_reads_2bit_host(gmx_engine *e, const uint64_t *stream, const uint64_t *offsets, uint32_t uniform_len, const uint32_t *seeds,
                            const uint8_t *skip, uint64_t n_reads) try {
  return map_reads_packed_impl(e, stream, true, offsets, uniform_len, seeds, skip, n_reads);
} GMX_GUARD_INT("gmx_map_reads_2bit_host")

void *gmx_engine_second_stream(gmx_engine *e) { return e && e->twin ? (void *)e->twin->main_stream : nullptr; }

int gmx_engine_seeds_in_place(gmx_engine *e, int on) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  e->seeds_in_place = on != 0;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_seeds_in_place")

int gmx_engine_sync_uploads(gmx_engine *e) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  if (e->copy_stream) {  // (sleeping, not polling: gmx_quiesce)
    if (!e->ev_wait) HIP_TRY(hipEventCreateWithFlags(&e->ev_wait, hipEventDisableTiming | hipEventBlockingSync));
    HIP_TRY(hipEventRecord(e->ev_wait, e->copy_stream));
    HIP_TRY(gmx_event_wait(e->ev_wait));
  }
  if (e->copy_stream2) {
    if (!e->ev_wait) HIP_TRY(hipEventCreateWithFlags(&e->ev_wait, hipEventDisableTiming | hipEventBlockingSync));
    HIP_TRY(hipEventRecord(e->ev_wait, e->copy_stream2));
    HIP_TRY(gmx_event_wait(e->ev_wait));
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_sync_uploads")

// page-locked allocations are remembered so that gmx_host_free knows which call returns them. Freed page-locked blocks
// of 1 MB or more are kept (up to 16 of them) and handed out again: pinning and unpinning 100 MB costs 10-20 ms each
// way, which a reads feed would otherwise pay at its start and again at its end.
static std::mutex g_host_mu;
struct HostBlock {
  uint64_t bytes;
  bool pinned;
};
static std::map<void *, HostBlock> g_host_live;
static std::vector<std::pair<void *, uint64_t>> g_host_spare;  // pinned blocks waiting for reuse
void *gmx_host_alloc(uint64_t bytes) try {
  bytes = std::max<uint64_t>(bytes, 1);
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    size_t best = g_host_spare.size();
    for (size_t i = 0; i < g_host_spare.size(); ++i)
      if (g_host_spare[i].second >= bytes && g_host_spare[i].second <= 2 * bytes + (1u << 20) &&
          (best == g_host_spare.size() || g_host_spare[i].second < g_host_spare[best].second))
        best = i;
    if (best != g_host_spare.size()) {
      void *p = g_host_spare[best].first;
      g_host_live[p] = HostBlock{g_host_spare[best].second, true};
      g_host_spare.erase(g_host_spare.begin() + (long)best);
      return p;
    }
  }
  void *p = nullptr;
  static const unsigned alloc_flags = getenv("GMX_HOST_ALLOC_FLAGS") ? (unsigned)strtoul(getenv("GMX_HOST_ALLOC_FLAGS"), nullptr, 0) : hipHostMallocDefault;
  bool pinned = hipHostMalloc(&p, bytes, alloc_flags) == hipSuccess && p;
  if (!pinned) {
    (void)hipGetLastError();
    p = malloc(bytes);
  }
  if (p) {
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_live[p] = HostBlock{bytes, pinned};
  }
  return p;
} GMX_GUARD_PTR("gmx_host_alloc")
void gmx_host_free(void *p) try {
  if (!p) return;
  HostBlock blk{0, false};
  {
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_live.find(p);
    if (it == g_host_live.end()) return;
    blk = it->second;
    g_host_live.erase(it);
    if (blk.pinned && blk.bytes >= (1u << 20) && g_host_spare.size() < 16) {
      g_host_spare.emplace_back(p, blk.bytes);
      return;
    }
  }
  if (blk.pinned)
    (void)hipHostFree(p);
  else
    free(p);
} GMX_GUARD_VOID("gmx_host_free")

// Sizes the batch workspace and the staging buffers of the _host entry point ahead of the first call (otherwise the first
// call allocates them, and a later, larger call allocates them again).
int gmx_engine_reserve(gmx_engine *e, uint64_t n_reads, uint64_t n_bases) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  n_reads = std::min<uint64_t>(n_reads, e->opts.max_batch_reads);
  e->allocs.room(4);  // (the bookkeeping of the four buffers below: short of host memory the call fails before it has changed anything)
  int rc = ensure_batch_capacity(e, n_reads);
  if (rc) return rc;
  const uint64_t need = n_bases / 32 + n_reads + 16;
  if ((rc = e->grow(e->packed, need, need, 0, true)) || (rc = e->grow(e->stage_reads, n_bases, n_bases, 16, true)) ||
      (rc = e->grow(e->stage_offsets, n_reads, n_reads, 1, true)) || (rc = e->grow(e->stage_seeds, n_reads, n_reads, 0, true)))
    return rc;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_reserve")

// The same for gmx_map_reads_packed_host: the batch workspace, the copy stream and the three upload slots (bit planes,
// offsets, seeds, skip flags) for chunks of up to n_reads reads / n_pairs plane pairs.
int gmx_engine_reserve_packed(gmx_engine *e, uint64_t n_reads, uint64_t n_pairs) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  n_reads = std::min<uint64_t>(n_reads, gmx_feed_chunk(e));
  int rc = ensure_batch_capacity(e, n_reads);
  if (rc) return rc;
  if (e->twin && (rc = ensure_batch_capacity(e->twin, n_reads))) return rc;
  if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  for (GmxFeedSlot *sl = e->slots + GMX_BYTE_SLOTS; sl != e->slots + GMX_BYTE_SLOTS + GMX_PACK_SLOTS; ++sl) {
    if (sl->busy) continue;  // (its batch is in flight: the feed sizes it when its turn comes)
    if ((rc = slot_acquire(*sl)) || (rc = slot_grow(e, *sl, SlotNeed{(n_pairs + 16) * 8, (n_pairs + 64) * 8, 0, n_reads, n_reads}, false))) return rc;
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_reserve_packed")

}  // extern "C"

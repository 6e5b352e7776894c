// gmx_engine_readback.h — part of gmx_engine.hip's translation unit (gmx_engine_state.h lists the parts): what comes back. Sync and
// the errors it reports, kernel timing, queue counts, the coverage on the device, through the exchange and on the host, the
// switches of the accumulator block's layout, the per-read logs, the grouped log's import and export.
#pragma once
extern "C" {

int gmx_engine_sync(gmx_engine *e) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  {
    int frc = flush_reset(e);
    if (frc) return frc;
    if ((frc = log_settle(e))) return frc;
  }
  {
    int qrc = gmx_quiesce(e);
    if (qrc) return qrc;
    if (e->twin && (qrc = gmx_quiesce(e->twin))) return qrc;
    e->twin_in_flight = false;
  }
  HIP_TRY(hipStreamSynchronize(e->last_stream));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t c[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpy(c + 2, e->d_error, 8, hipMemcpyDeviceToHost));
  if (c[2] == 0 && e->twin) {  // (the twin's batches report in its own words)
    HIP_TRY(hipMemcpy(c + 2, e->twin->d_error, 8, hipMemcpyDeviceToHost));
    if (c[2] != 0) HIP_TRY(hipMemset(e->twin->d_error, 0, 8));
  }
  if (c[2] != 0) {
    HIP_TRY(hipMemset(e->d_error, 0, 8));
    char msg[256];
    if (c[2] == GMX_TASK_LOGFULL) {
      snprintf(msg, sizeof(msg),
               "a read's records exceed the whole grouped-allele-count log (sites without dense group counters; %u words): "
               "nothing of it was recorded: raise gmx_engine_opts.log_cap_words",
               e->log_cap);
      gmx_set_error(msg);
      return GMX_ECAP;
    }
    if (c[2] == GMX_TASK_OVERFLOW) {
      snprintf(msg, sizeof(msg),
               "read %u (orientation %u) needs more memory for its search states or its mapping instances than the whole "
               "last-tier heap holds (%llu bytes); nothing of this read was recorded: raise gmx_engine_opts.huge_heap_bytes "
               "(GMX_HUGE_HEAP_BYTES)",
               c[3] >> 1, c[3] & 1, (unsigned long long)e->heap_words * 4);
      gmx_set_error(msg);
      return GMX_ECAP;
    }
    snprintf(msg, sizeof(msg),
             "read %u (orientation %u): inconsistent variant path (the reference throws/asserts here: a site "
             "traversed twice or an exit that does not match the entered site)",
             c[3] >> 1, c[3] & 1);
    gmx_set_error(msg);
    return GMX_EREF;
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_sync")

int gmx_engine_enable_timing(gmx_engine *e, int on) try {
  e->timing = on != 0;
  if (e->twin) e->twin->timing = e->timing;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_enable_timing")

int gmx_engine_timing(gmx_engine *e, gmx_timing *out) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  if (e->twin) {  // (the twin's batches: its events, added to this engine's sums)
    e->pending.insert(e->pending.end(), e->twin->pending.begin(), e->twin->pending.end());
    e->twin->pending.clear();
  }
  for (auto &ev : e->pending) {
    HIP_TRY(hipEventSynchronize(ev.c));
    float ms0 = 0, ms1 = 0, ms2 = 0;
    HIP_TRY(hipEventElapsedTime(&ms0, ev.s, ev.a));
    HIP_TRY(hipEventElapsedTime(&ms1, ev.a, ev.b));
    HIP_TRY(hipEventElapsedTime(&ms2, ev.b, ev.c));
    e->search_ms += ms1;
    e->cover_ms += ms0 + ms2;
    e->search_launches++;
    e->cover_launches++;
    e->timed_reads += ev.reads;
    for (int k = 0; k < GMX_TK_N; ++k) {
      if (ev.timed & (1u << k)) {  // (events of other streams: complete, ev.c is behind the batch's join)
        float ms = 0;
        HIP_TRY(hipEventSynchronize(ev.k[k][1]));
        HIP_TRY(hipEventElapsedTime(&ms, ev.k[k][0], ev.k[k][1]));
        e->kernel_ms[k] += ms;
        e->kernel_launches[k]++;
      }
      (void)hipEventDestroy(ev.k[k][0]);
      (void)hipEventDestroy(ev.k[k][1]);
    }
    (void)hipEventDestroy(ev.s);
    (void)hipEventDestroy(ev.a);
    (void)hipEventDestroy(ev.b);
    (void)hipEventDestroy(ev.c);
  }
  e->pending.clear();
  out->search_ms = e->search_ms;
  out->search_launches = e->search_launches;
  out->cover_ms = e->cover_ms;
  out->cover_launches = e->cover_launches;
  out->reads = e->timed_reads;
  for (int k = 0; k < GMX_TIMED_KERNELS; ++k) {
    out->kernel_ms[k] = e->kernel_ms[k];
    out->kernel_launches[k] = e->kernel_launches[k];
    e->kernel_ms[k] = 0;
    e->kernel_launches[k] = 0;
  }
  e->search_ms = e->cover_ms = 0;
  e->search_launches = e->cover_launches = e->timed_reads = 0;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_timing")

int gmx_engine_queue_counts(gmx_engine *e, gmx_queue_counts *out) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t raw[GMX_N_COUNTERS * GMX_CNT_STRIDE];
  HIP_TRY(hipMemcpy(raw, (e->twin && e->last_on_twin ? e->twin : e)->d_counters, sizeof(raw), hipMemcpyDeviceToHost));  // (the workspace of the LAST launch)
  auto c = [&](int i) { return (uint64_t)raw[i * GMX_CNT_STRIDE]; };
  out->mapped = 0;
  for (int r = 0; r < GMX_REGIONS; ++r) out->mapped += c(16 + r);
  out->mapped += c(8);
  out->alive = c(5);
  out->dead = c(6) + c(12);
  out->overflow_probe = c(1);
  out->overflow_extend = c(9);
  out->big_mapped = c(7);
  out->cover_general = c(8);
  out->cover_mid = c(13);
  out->cover_overflow = c(4);
  out->seed_cursor = e->seed_cursor ? 1 : 0;
  out->inst_mapped = c(25);
  out->huge_search = c(11);
  out->huge_cover = c(15);
  out->log_replays = e->log_replays;
  out->log_replayed_entries = e->log_replayed_entries;
  out->overflow_split = c(29);
  out->coop_rejected = c(26) + c(27) + c(28);
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_queue_counts")

int gmx_debug_straggler_counts(gmx_engine *e, uint64_t out[3]) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  HIP_TRY(hipDeviceSynchronize());
  static_assert(GMX_EXTRA_PASSES == 3, "gmx_debug_straggler_counts: one count per straggler list");
  uint32_t raw[GMX_N_COUNTERS * GMX_CNT_STRIDE];
  HIP_TRY(hipMemcpy(raw, (e->twin && e->last_on_twin ? e->twin : e)->d_counters, sizeof(raw), hipMemcpyDeviceToHost));  // (the workspace of the LAST launch)
  for (uint32_t pass = 0; pass < GMX_EXTRA_PASSES; ++pass) out[pass] = raw[(GMX_CNT_ALIVE2 + pass) * GMX_CNT_STRIDE];
  return GMX_OK;
} GMX_GUARD_INT("gmx_debug_straggler_counts")

// The coverage ladder's queue lengths one by one (gmx_engine_queue_counts sums some of them and leaves others out): only what
// the kernels of the LAST launch wrote anyway. The order is that of gmx.h.
int gmx_debug_cover_counts(gmx_engine *e, uint64_t out[12]) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  HIP_TRY(hipDeviceSynchronize());
  uint32_t raw[GMX_N_COUNTERS * GMX_CNT_STRIDE];
  HIP_TRY(hipMemcpy(raw, (e->twin && e->last_on_twin ? e->twin : e)->d_counters, sizeof(raw), hipMemcpyDeviceToHost));  // (the workspace of the LAST launch)
  static const uint32_t which[12] = {8u, GMX_CNT_GENERAL_REST, 27u, 26u, 28u, 13u, 4u, 15u, 11u, 7u, 25u, GMX_CNT_TAIL_RETRY};
  for (int i = 0; i < 12; ++i) out[i] = raw[which[i] * GMX_CNT_STRIDE];
  return GMX_OK;
} GMX_GUARD_INT("gmx_debug_cover_counts")

int gmx_coverage_device(gmx_engine *e, gmx_device_coverage *out) try {
  {
    int frc = flush_reset(e);
    if (frc) return frc;
  }
  if (e->twin && e->twin_in_flight) {  // (the caller is about to read the block: the twin's batches first)
    int qrc = gmx_quiesce(e->twin);
    if (qrc) return qrc;
    e->twin_in_flight = false;
  }
  out->allele_sum = out->per_base = out->grouped = nullptr;  // interleaved in the block: use `fused`, or gmx_coverage_fetch
  out->n_allele_sum = e->n_allele;
  out->n_per_base = e->n_pb;
  out->n_grouped = e->n_grouped;
  out->stats = e->d_stats;
  out->n_stats = 5;
  out->fused = e->d_fused;
  out->n_fused = e->n_fused;
  return GMX_OK;
} GMX_GUARD_INT("gmx_coverage_device")

int gmx_coverage_reduce_begin(gmx_engine *e, void *hip_stream) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  {
    int frc = flush_reset(e);
    if (frc) return frc;
    if ((frc = log_settle(e))) return frc;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  {
    int trc = twin_join(e, (hipStream_t)hip_stream);  // (the exchange reads what the twin's batches record)
    if (trc) return trc;
  }
  e->recorded = true;  // (what the exchange adds to the block)
  hipLaunchKernelGGL(gmx_stats_limbs_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, e->d_stats, e->d_limbs, 0);
  HIP_TRY(hipGetLastError());
  return GMX_OK;
} GMX_GUARD_INT("gmx_coverage_reduce_begin")

int gmx_coverage_reduce_end(gmx_engine *e, void *hip_stream) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  {
    int frc = flush_reset(e);
    if (frc) return frc;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  hipLaunchKernelGGL(gmx_stats_limbs_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, e->d_stats, e->d_limbs, 1);
  HIP_TRY(hipGetLastError());
  return GMX_OK;
} GMX_GUARD_INT("gmx_coverage_reduce_end")

// one accumulator block -> the three logical arrays, ADDED to them (the gather of gmx_coverage_fetch; any pointer may be null)
static void gather_block(const gmx_engine *e, const uint32_t *block, uint32_t *allele_sum, uint32_t *per_base, uint32_t *grouped) {
  if (allele_sum) for (size_t i = 0; i < e->phys_allele.size(); ++i) allele_sum[i] += block[e->phys_allele[i]];
  if (per_base) for (size_t i = 0; i < e->phys_pb.size(); ++i) per_base[i] += block[e->phys_pb[i]];
  if (grouped) for (size_t i = 0; i < e->phys_grouped.size(); ++i) grouped[i] += block[e->phys_grouped[i]];
  for (size_t i = 0; i + 3 < e->hit_fix.size(); i += 4) {  // a hit = one each of allele-sum, group {allele} and the base
    const uint32_t hits = block[e->hit_fix[i]];
    if (allele_sum) allele_sum[e->hit_fix[i + 1]] += hits;
    if (grouped) grouped[e->hit_fix[i + 2]] += hits;
    if (per_base) per_base[e->hit_fix[i + 3]] += hits;
  }
}
// blocks [first, first + count) of the engine, gathered and added up (uint32 wrap) into zeroed outputs
static int fetch_blocks(gmx_engine *e, size_t first, size_t count, uint32_t *allele_sum, uint32_t *per_base, uint32_t *grouped) {
  {
    int frc = flush_reset(e);
    if (frc) return frc;
    if ((frc = log_settle(e))) return frc;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  HIP_TRY(hipDeviceSynchronize());
  if (!allele_sum && !per_base && !grouped) return GMX_OK;  // (a caller after the read counters alone: no block to copy)
  std::vector<uint32_t> block(std::max<size_t>(e->n_acc * count, 1));
  if (e->n_acc) HIP_TRY(hipMemcpy(block.data(), e->d_fused + first * e->n_acc, e->n_acc * count * 4, hipMemcpyDeviceToHost));
  if (allele_sum) std::fill(allele_sum, allele_sum + e->phys_allele.size(), 0u);
  if (per_base) std::fill(per_base, per_base + e->phys_pb.size(), 0u);
  if (grouped) std::fill(grouped, grouped + e->phys_grouped.size(), 0u);
  for (size_t k = 0; k < count; ++k) gather_block(e, block.data() + k * e->n_acc, allele_sum, per_base, grouped);
  return GMX_OK;
}

int gmx_coverage_fetch(gmx_engine *e, uint32_t *allele_sum, uint32_t *per_base, uint32_t *grouped, gmx_stats *stats) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  {  // (per strand: the totals are both blocks added)
    int rc = fetch_blocks(e, 0, e->record_strands ? 2 : 1, allele_sum, per_base, grouped);
    if (rc) return rc;
  }
  if (stats) {
    unsigned long long s[5];
    HIP_TRY(hipMemcpy(s, e->d_stats, sizeof(s), hipMemcpyDeviceToHost));
    stats->all_reads_count = s[0];
    stats->skipped_reads_count = s[1];
    stats->missing_kmer_reads_count = s[2];
    stats->no_extension_reads_count = s[3];
    stats->exact_mapped_reads_count = s[4];
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_coverage_fetch")

int gmx_coverage_fetch_strand(gmx_engine *e, int strand, uint32_t *allele_sum, uint32_t *per_base, uint32_t *grouped_dense) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  if (!e->record_strands) {
    gmx_set_error("gmx_coverage_fetch_strand: the engine does not record per strand (gmx_engine_record_strands)");
    return GMX_EINVAL;
  }
  if (strand != 0 && strand != 1) {
    gmx_set_error("gmx_coverage_fetch_strand: strand is 0 (forward) or 1 (reverse complement)");
    return GMX_EINVAL;
  }
  return fetch_blocks(e, (size_t)strand, 1, allele_sum, per_base, grouped_dense);
} GMX_GUARD_INT("gmx_coverage_fetch_strand")

// The engine's one-block or two-block allocation. Nothing is recorded and nothing is in flight when this runs, so the new
// block is simply a zeroed one; the old one stays untouched until the new one exists.
// Layout of the fused block: [block] or [forward block | reverse block], then [tally: 2 * n_sites words rounded up to 64] when the
// per-site ambiguity counts are on, then [links: off[n_sites] words rounded up to 64] when links are recorded, then the 32 limb
// words; 16 words of read counters and the log cursor behind it.
static int set_block_layout(gmx_engine *e, bool strands, bool site_ambiguity, int span, const char *who) {
  if (e->record_strands == strands && e->record_site_ambiguity == site_ambiguity && e->link_span == span) return GMX_OK;
  const size_t n_tally = site_ambiguity ? (2 * (size_t)e->dview.n_sites + 63) / 64 * 64 : 0;
  // the link block (gmx_link.h): its size and the per-site words follow from the index and the span alone — one scan of the sites
  size_t n_links = 0;
  std::vector<GmxLinkSite> table;
  if (span) {
    if (e->dview.is_nested) {
      gmx_set_error(std::string(who) + ": links are recorded on flat PRGs only (the distance between two sites is not defined across the levels of a nested PRG)");
      return GMX_EINVAL;
    }
    const size_t n_sites = e->link_alleles.size();
    std::vector<uint64_t> off(n_sites + 1);
    gmx_link_offsets(n_sites, (uint32_t)span, [&](uint64_t s) { return (uint32_t)e->link_alleles[s]; }, off.data());
    if (off[n_sites] > 0xFFFFFFFFull) {
      gmx_set_error(std::string(who) + ": the link block of this index and span exceeds 2^32 words");
      return GMX_EINVAL;
    }
    n_links = (size_t)off[n_sites];
    if (span != e->link_span) {
      table.resize(n_sites);
      for (size_t s = 0; s < n_sites; ++s) {
        uint32_t f = 0;
        for (size_t k = 0; k < 8 && s + k < n_sites; ++k) f |= (uint32_t)e->link_alleles[s + k] << (4 * k);
        table[s] = GmxLinkSite{(uint32_t)off[s], f};
      }
    }
  }
  const size_t n_fused = (strands ? 2 : 1) * e->n_acc + n_tally + (n_links + 63) / 64 * 64 + 32;
  if (n_fused + 32 > 0xFFFFFFFFull) {  // (the resets' word counts and CoverAcc::rev_off are 32 bits)
    gmx_set_error(std::string(who) + ": the accumulator blocks of this index exceed 2^32 words");
    return GMX_EINVAL;
  }
  uint32_t *old = e->d_fused, *q = nullptr;
  int rc = e->alloc(&q, n_fused + 32, true);  // + 16 words of read counters + log cursor
  if (rc) return rc;
  GmxLinkSite *old_sites = e->d_link_sites, *sites = span == e->link_span ? old_sites : nullptr;
  if (span && span != e->link_span) {  // (the old block and mode stay when this fails)
    rc = e->alloc(&sites, table.size(), false);
    if (!rc && !table.empty() && hipMemcpy(sites, table.data(), table.size() * sizeof(GmxLinkSite), hipMemcpyHostToDevice) != hipSuccess) {
      gmx_set_error(std::string(who) + ": the per-site words could not be copied to the device");
      rc = GMX_EHIP;
    }
    if (rc) {
      e->release(sites);
      e->release(q);
      return rc;
    }
  }
  e->release(old);
  if (sites != old_sites) e->release(old_sites);
  e->record_strands = strands;
  e->record_site_ambiguity = site_ambiguity;
  e->n_tally = n_tally;
  e->link_span = span;
  e->n_links = n_links;
  e->d_link_sites = sites;
  e->reset_pending = false;  // (a queued reset: the fresh block is zero)
  for (gmx_engine *w : {e, e->twin}) {  // the twin's alias of the block and every derived pointer follow
    if (!w) continue;
    w->d_fused = q;
    w->n_fused = n_fused;
    w->d_limbs = q + n_fused - 32;
    w->d_stats = reinterpret_cast<unsigned long long *>(q + n_fused);
    w->d_log_cursor = q + n_fused + 16;
  }
  return GMX_OK;
}
static int set_record_strands(gmx_engine *e, bool on) { return set_block_layout(e, on, e->record_site_ambiguity, e->link_span, "gmx_engine_record_strands"); }
static int set_record_site_ambiguity(gmx_engine *e, bool on) {
  return set_block_layout(e, e->record_strands, on, e->link_span, "gmx_engine_record_site_ambiguity");
}
static int set_record_links(gmx_engine *e, int span) {
  if (span < 0 || span > (int)GMX_LINK_MAX_SPAN) {
    gmx_set_error("gmx_engine_record_links: span is 0 (off) to " + std::to_string(GMX_LINK_MAX_SPAN) + ", not " + std::to_string(span));
    return GMX_EINVAL;
  }
  return set_block_layout(e, e->record_strands, e->record_site_ambiguity, span, "gmx_engine_record_links");
}

// The C ABI of a switch of the block's layout: only while nothing is recorded
static int block_layout_switch(gmx_engine *e, int (*set)(gmx_engine *, int), int arg, const char *who) {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  if (e->recorded) {
    gmx_set_error(std::string(who) + ": coverage has been recorded since the last reset (call gmx_engine_reset first)");
    return GMX_EINVAL;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  HIP_TRY(hipDeviceSynchronize());  // the engine's work (a reset still queued is dropped: the fresh block is zero)
  return set(e, arg);
}

int gmx_engine_record_strands(gmx_engine *e, int on) try {
  return block_layout_switch(e, [](gmx_engine *w, int v) { return set_record_strands(w, v != 0); }, on, "gmx_engine_record_strands");
} GMX_GUARD_INT("gmx_engine_record_strands")

int gmx_engine_record_site_ambiguity(gmx_engine *e, int on) try {
  return block_layout_switch(e, [](gmx_engine *w, int v) { return set_record_site_ambiguity(w, v != 0); }, on, "gmx_engine_record_site_ambiguity");
} GMX_GUARD_INT("gmx_engine_record_site_ambiguity")

int gmx_engine_site_ambiguity(gmx_engine *e) try {
  return e && e->record_site_ambiguity ? 1 : 0;
} GMX_GUARD_ZERO("gmx_engine_site_ambiguity")

int gmx_coverage_fetch_site_ambiguity(gmx_engine *e, uint32_t *drawn, uint32_t *passed, uint64_t n_sites) try {
  if (!e || (n_sites && (!drawn || !passed))) {
    gmx_set_error("gmx_coverage_fetch_site_ambiguity: null argument");
    return GMX_EINVAL;
  }
  if (!e->record_site_ambiguity) {
    gmx_set_error("gmx_coverage_fetch_site_ambiguity: the engine does not record them (gmx_engine_record_site_ambiguity)");
    return GMX_EINVAL;
  }
  if (n_sites != e->dview.n_sites) {
    gmx_set_error("gmx_coverage_fetch_site_ambiguity: n_sites is " + std::to_string(n_sites) + ", the index has " + std::to_string(e->dview.n_sites));
    return GMX_EINVAL;
  }
  {  // (a task redone after a full log counts then; both workspaces' streams)
    int rc = fetch_blocks(e, 0, 0, nullptr, nullptr, nullptr);
    if (rc) return rc;
  }
  std::vector<uint32_t> w(std::max<size_t>(2 * (size_t)n_sites, 1));
  if (n_sites) HIP_TRY(hipMemcpy(w.data(), e->d_fused + e->tally_off(), 2 * (size_t)n_sites * 4, hipMemcpyDeviceToHost));
  for (size_t s = 0; s < n_sites; ++s) {
    drawn[s] = w[2 * s];
    passed[s] = w[2 * s + 1];
  }
  return GMX_OK;
} GMX_GUARD_INT("gmx_coverage_fetch_site_ambiguity")

// Links between nearby sites: the switch follows the rule of the two above; the span is the mode.
int gmx_engine_record_links(gmx_engine *e, int span) try {
  return block_layout_switch(e, set_record_links, span, "gmx_engine_record_links");
} GMX_GUARD_INT("gmx_engine_record_links")

int gmx_engine_links(gmx_engine *e) try {
  return e ? e->link_span : 0;
} GMX_GUARD_ZERO("gmx_engine_links")

int gmx_coverage_fetch_links(gmx_engine *e, uint32_t *words, uint64_t n_words) try {
  if (!e || (n_words && !words)) {
    gmx_set_error("gmx_coverage_fetch_links: null argument");
    return GMX_EINVAL;
  }
  if (!e->link_span) {
    gmx_set_error("gmx_coverage_fetch_links: the engine does not record them (gmx_engine_record_links)");
    return GMX_EINVAL;
  }
  if (n_words != e->n_links) {
    gmx_set_error("gmx_coverage_fetch_links: n_words is " + std::to_string(n_words) + ", the layout of this index and span has " + std::to_string(e->n_links) +
                  " (gmx_index_link_layout)");
    return GMX_EINVAL;
  }
  {  // (a task redone after a full log counts then; both workspaces' streams)
    int rc = fetch_blocks(e, 0, 0, nullptr, nullptr, nullptr);
    if (rc) return rc;
  }
  if (n_words) HIP_TRY(hipMemcpy(words, e->d_fused + e->links_off(), (size_t)n_words * 4, hipMemcpyDeviceToHost));
  return GMX_OK;
} GMX_GUARD_INT("gmx_coverage_fetch_links")

// The limit on a selection's candidates: a launch argument of the coverage kernels (CoverAcc::max_candidates), nothing to allocate.
// Only while nothing is recorded: the coverage of one job is that of ONE limit, and a task redone after a full log or run on the
// twin workspace meets the value of its first pass.
int gmx_engine_set_max_candidates(gmx_engine *e, uint32_t limit) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  if (e->recorded) {
    gmx_set_error("gmx_engine_set_max_candidates: coverage has been recorded since the last reset (call gmx_engine_reset first)");
    return GMX_EINVAL;
  }
  e->max_candidates = limit;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_set_max_candidates")

uint32_t gmx_engine_max_candidates(gmx_engine *e) try {
  return e ? e->max_candidates : 0u;
} GMX_GUARD_ZERO("gmx_engine_max_candidates")

// The C ABI of a per-read log, shared by the outcome bytes and the position records.
static int read_log_record(gmx_engine *e, GmxReadLog gmx_engine::*log, int on) {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  (e->*log).on = on != 0;
  return GMX_OK;
}

static int64_t read_log_count(gmx_engine *e, GmxReadLog gmx_engine::*log) {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  return (int64_t)(e->*log).count;
}

// reads first .. first + n of the log into `out`, once everything handed over has left its record (`name`: the caller's, for the
// error texts)
static int read_log_fetch(gmx_engine *e, GmxReadLog gmx_engine::*which, uint64_t first, uint64_t n, void *out, const char *name) {
  if (!e || (n && !out)) {
    gmx_set_error(std::string(name) + ": null argument");
    return GMX_EINVAL;
  }
  const GmxReadLog &log = e->*which;
  if (first > log.count || n > log.count - first) {
    gmx_set_error(std::string(name) + ": reads " + std::to_string(first) + " .. " + std::to_string(first + n) + " of " +
                  std::to_string(log.count) + " recorded");
    return GMX_EINVAL;
  }
  {
    int frc = flush_reset(e);
    if (frc) return frc;
    if ((frc = log_settle(e))) return frc;  // (a task redone after a full log leaves its bits and its record then)
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  HIP_TRY(hipDeviceSynchronize());  // both workspaces' streams
  if (n) HIP_TRY(hipMemcpy(out, reinterpret_cast<const uint8_t *>(log.d) + first * log.stride, n * log.stride, hipMemcpyDeviceToHost));
  return GMX_OK;
}

int gmx_engine_record_outcomes(gmx_engine *e, int on) try {
  return read_log_record(e, &gmx_engine::outcomes, on);
} GMX_GUARD_INT("gmx_engine_record_outcomes")

int64_t gmx_engine_outcome_count(gmx_engine *e) try {
  return read_log_count(e, &gmx_engine::outcomes);
} GMX_GUARD_INT("gmx_engine_outcome_count")

int gmx_engine_fetch_outcomes(gmx_engine *e, uint64_t first, uint64_t n, uint8_t *out) try {
  return read_log_fetch(e, &gmx_engine::outcomes, first, n, out, "gmx_engine_fetch_outcomes");
} GMX_GUARD_INT("gmx_engine_fetch_outcomes")

// Counted records of e->log_counts into `out` (as far as they fit) and their length in words: one strand's counts, their sums,
// or the exchange form (up to two records per key, the reverse one with GMX_LOG_REVERSE).
enum LogForm { LOG_FORWARD = 0, LOG_REVERSE_ONLY = 1, LOG_TOTALS = 2, LOG_EXCHANGE = 3 };
// what engines pass to each other: without strands every count is a forward one, the records of the totals
static LogForm exchange_form(const gmx_engine *e) { return e->record_strands ? LOG_EXCHANGE : LOG_TOTALS; }
static uint64_t emit_log_counts(const gmx_engine *e, LogForm which, uint32_t *out, uint64_t cap_words) {
  uint64_t n = 0;
  for (auto const &kv : e->log_counts) {  // [site_index, n_ids | GMX_LOG_COUNTED, count lo, count hi, ids...]
    const uint64_t words = 4 + (kv.first.size() - 1);
    for (int s = 0; s < (which == LOG_EXCHANGE ? 2 : 1); ++s) {
      const uint64_t count = which == LOG_TOTALS ? kv.second[0] + kv.second[1] : kv.second[which == LOG_EXCHANGE ? s : which];
      if (!count) continue;
      if (out && n + words <= cap_words) {
        out[n] = kv.first[0];
        out[n + 1] = (uint32_t)(kv.first.size() - 1) | GMX_LOG_COUNTED | (which == LOG_EXCHANGE && s ? GMX_LOG_REVERSE : 0u);
        out[n + 2] = (uint32_t)count;
        out[n + 3] = (uint32_t)(count >> 32);
        for (size_t j = 1; j < kv.first.size(); ++j) out[n + 3 + j] = kv.first[j];
      }
      n += words;
    }
  }
  return n;
}

int gmx_engine_record_positions(gmx_engine *e, int on) try {
  return read_log_record(e, &gmx_engine::positions, on);
} GMX_GUARD_INT("gmx_engine_record_positions")

int64_t gmx_engine_position_count(gmx_engine *e) try {
  return read_log_count(e, &gmx_engine::positions);
} GMX_GUARD_INT("gmx_engine_position_count")

int gmx_engine_fetch_positions(gmx_engine *e, uint64_t first, uint64_t n, uint32_t *out) try {
  return read_log_fetch(e, &gmx_engine::positions, first, n, out, "gmx_engine_fetch_positions");
} GMX_GUARD_INT("gmx_engine_fetch_positions")

int64_t gmx_coverage_fetch_grouped_log(gmx_engine *e, uint32_t *out, uint64_t cap_words) try {
  if (!e) return GMX_EINVAL;
  if (hipSetDevice(e->opts.device) != hipSuccess) return GMX_EHIP;
  if (log_settle(e)) return GMX_EHIP;
  if (gmx_log_drain(e, 0)) return GMX_EHIP;
  return (int64_t)emit_log_counts(e, LOG_TOTALS, out, cap_words);
} GMX_GUARD_INT("gmx_coverage_fetch_grouped_log")

int64_t gmx_coverage_fetch_grouped_log_strand(gmx_engine *e, int strand, uint32_t *out, uint64_t cap_words) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  if (!e->record_strands) {
    gmx_set_error("gmx_coverage_fetch_grouped_log_strand: the engine does not record per strand (gmx_engine_record_strands)");
    return GMX_EINVAL;
  }
  if (strand != 0 && strand != 1) {
    gmx_set_error("gmx_coverage_fetch_grouped_log_strand: strand is 0 (forward) or 1 (reverse complement)");
    return GMX_EINVAL;
  }
  if (hipSetDevice(e->opts.device) != hipSuccess) return GMX_EHIP;
  if (log_settle(e)) return GMX_EHIP;
  if (gmx_log_drain(e, 0)) return GMX_EHIP;
  return (int64_t)emit_log_counts(e, strand ? LOG_REVERSE_ONLY : LOG_FORWARD, out, cap_words);
} GMX_GUARD_INT("gmx_coverage_fetch_grouped_log_strand")

int64_t gmx_coverage_export_grouped_log(gmx_engine *e, uint32_t *out, uint64_t cap_words) try {
  if (!e) {
    gmx_set_error("null engine");
    return GMX_EINVAL;
  }
  if (hipSetDevice(e->opts.device) != hipSuccess) return GMX_EHIP;
  if (log_settle(e)) return GMX_EHIP;
  if (gmx_log_drain(e, 0)) return GMX_EHIP;
  return (int64_t)emit_log_counts(e, exchange_form(e), out, cap_words);
} GMX_GUARD_INT("gmx_coverage_export_grouped_log")

int gmx_coverage_import_grouped_log(gmx_engine *e, const uint32_t *records, uint64_t n_words, int replace) try {
  if (!e || (!records && n_words)) {
    gmx_set_error("gmx_coverage_import_grouped_log: null argument");
    return GMX_EINVAL;
  }
  {
    int frc = flush_reset(e);
    if (frc) return frc;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  return gmx_engine_log_import(e, records, (size_t)n_words, replace != 0);
} GMX_GUARD_INT("gmx_coverage_import_grouped_log")

}  // extern "C"

uint64_t gmx_engine_reset_epoch(const gmx_engine *e) { return e->reset_epoch; }

void gmx_engine_raw(gmx_engine *e, GmxEngineRaw *out) {
  (void)flush_reset(e);
  out->device = e->opts.device;
  out->d_fused = e->d_fused;
  out->n_fused = e->n_fused;
  out->log_sites = e->log_sites;
  out->record_strands = e->record_strands;
  out->record_site_ambiguity = e->record_site_ambiguity;
  out->link_span = e->link_span;
}

int gmx_engine_log_export(gmx_engine *e, std::vector<uint32_t> &out) {
  {
    int frc = flush_reset(e);
    if (frc) return frc;
    if ((frc = log_settle(e))) return frc;
  }
  HIP_TRY(hipSetDevice(e->opts.device));
  {
    int rc = gmx_log_drain(e, 0);
    if (rc) return rc;
  }
  const LogForm which = exchange_form(e);
  out.assign((size_t)emit_log_counts(e, which, nullptr, 0), 0);
  emit_log_counts(e, which, out.data(), out.size());
  return GMX_OK;
}

int gmx_engine_log_import(gmx_engine *e, const uint32_t *w, size_t n_words, bool replace) {
  {
    int frc = flush_reset(e);
    if (frc) return frc;
  }
  const uint32_t flags = GMX_LOG_COUNTED | GMX_LOG_REVERSE;
  for (size_t i = 0; i < n_words;) {  // all of it is checked before any of it counts
    if (w[i] == GMX_LOG_PAD) {
      ++i;
      continue;
    }
    if (i + 2 > n_words) break;
    const uint32_t n = w[i + 1] & ~flags;
    const size_t head = (w[i + 1] & GMX_LOG_COUNTED) ? 4 : 2;
    if (i + head + n > n_words) {
      gmx_set_error("corrupt grouped log");
      return GMX_EINVAL;
    }
    if ((w[i + 1] & GMX_LOG_REVERSE) && !e->record_strands) {
      gmx_set_error("grouped log: a reverse-complement record (GMX_LOG_REVERSE) for an engine that does not record per strand");
      return GMX_EINVAL;
    }
    i += head + n;
  }
  if (replace) {
    int rc = gmx_log_drain(e, 0);  // whatever is still on the device belongs to the totals being replaced
    if (rc) return rc;
    e->log_counts.clear();
  }
  std::vector<uint32_t> key;
  for (size_t i = 0; i < n_words;) {
    if (w[i] == GMX_LOG_PAD) {
      ++i;
      continue;
    }
    if (i + 2 > n_words) break;
    const uint32_t n = w[i + 1] & ~flags;
    const size_t head = (w[i + 1] & GMX_LOG_COUNTED) ? 4 : 2;
    const uint64_t count = head == 4 ? ((uint64_t)w[i + 2] | ((uint64_t)w[i + 3] << 32)) : 1;
    key.assign(1, w[i]);
    key.insert(key.end(), w + i + head, w + i + head + n);
    e->log_counts[key][(w[i + 1] & GMX_LOG_REVERSE) ? 1 : 0] += count;
    i += head + n;
  }
  return GMX_OK;
}

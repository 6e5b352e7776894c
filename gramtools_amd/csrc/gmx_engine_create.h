// gmx_engine_create.h — part of gmx_engine.hip's translation unit (gmx_engine_state.h lists the parts): an engine's default options,
// the device copy of an index shared by the engines on one device, creation and destruction, the two resets.
#pragma once
extern "C" {

void gmx_engine_default_opts(gmx_engine_opts *o) try {
  o->device = 0;
  o->rng_mode = GMX_RNG_LEMIRE;
  o->max_states = 1024;
  o->max_path_nodes = 2048;
  o->max_batch_reads = 4u << 20;
  o->forward_only = 0;
  o->huge_heap_bytes = 512ull << 20;
  o->log_cap_words = 0;
} GMX_GUARD_VOID("gmx_engine_default_opts")

// The device copy of an index is shared by the engines made of it on one device (round 5): several engines per GPU keep batches
// in flight side by side — a nested PRG's batch is a 0.4 ms burst and then 2 ms of a few straggler tasks on a handful of CUs —
// and the second one must not cost a second upload and a second copy in HBM. Reference counted; GMX_NO_INDEX_SHARE=1: off.
struct GmxDeviceIndex {
  uint64_t serial = 0;  // gmx_index_serial of the index it was uploaded from
  int device = 0;
  GmxIndexView view{};
  GmxAllocs allocs;
  uint64_t bytes = 0;
  int refs = 0;
};
static std::mutex g_dev_index_mu;
static std::vector<GmxDeviceIndex *> g_dev_indexes;
static void gmx_dev_index_release(GmxDeviceIndex *d) {
  if (!d) return;
  std::lock_guard<std::mutex> lk(g_dev_index_mu);
  if (--d->refs > 0) return;
  d->allocs.release_all();
  g_dev_indexes.erase(std::remove(g_dev_indexes.begin(), g_dev_indexes.end(), d), g_dev_indexes.end());
  delete d;
}

static int engine_create(const gmx_index *ixh, const gmx_engine_opts *opts_in, gmx_engine *primary, gmx_engine **out);
static int set_record_strands(gmx_engine *e, bool on);
static int set_record_site_ambiguity(gmx_engine *e, bool on);
static int set_record_links(gmx_engine *e, int span);
int gmx_engine_create(const gmx_index *ixh, const gmx_engine_opts *opts_in, gmx_engine **out) try {
  int rc = engine_create(ixh, opts_in, nullptr, out);
  if (rc) return rc;
  gmx_engine *e = *out;
  // MEASUREMENT HOOK ONLY (profiles/read_outcomes: the cost of recording in an unchanged benchmark): nothing reads the bytes back
  if (const char *ro = getenv("GMX_RECORD_OUTCOMES")) e->outcomes.on = atoi(ro) != 0;
  if (const char *rp = getenv("GMX_RECORD_POSITIONS")) e->positions.on = atoi(rp) != 0;  // (the same kind: profiles/read_positions)
  // the twin (a second batch in flight; gmx_engine::twin): nested PRGs and indexes of 2 GB and more
  const gmx::HostIndex &h = gmx_index_host(ixh);
  const bool can = !e->log_sites && e->shared_index && !getenv("GMX_NO_INDEX_SHARE");  // (the twin reads the engine's copy of the index, never one of its own)
  bool want = can && (h.is_nested || e->index_bytes >= (2ull << 30));
  if (const char *tw = getenv("GMX_TWIN")) want = can && atoi(tw) != 0;
  if (want) {
    gmx_engine *t = nullptr;
    if (engine_create(ixh, &e->opts, e, &t) == GMX_OK) {
      e->twin = t;
      t->owner = e;
    } else {
      (void)hipGetLastError();  // (no room for a second workspace: one batch at a time, as before)
    }
  }
  // MEASUREMENT HOOK ONLY (profiles/strand_coverage: the cost of two blocks in an unchanged benchmark): nothing reads them apart
  if (const char *rs = getenv("GMX_RECORD_STRANDS"))
    if (atoi(rs) != 0 && (rc = set_record_strands(e, true))) {
      gmx_engine_destroy(e);
      *out = nullptr;
      return rc;
    }
  // MEASUREMENT HOOK ONLY (profiles/site_ambiguity: the cost of the per-site counts in an unchanged benchmark): nothing reads them
  if (const char *sa = getenv("GMX_RECORD_SITE_AMBIGUITY"))
    if (atoi(sa) != 0 && (rc = set_record_site_ambiguity(e, true))) {
      gmx_engine_destroy(e);
      *out = nullptr;
      return rc;
    }
  // MEASUREMENT HOOK ONLY (profiles/site_links: the cost of the links in an unchanged benchmark; flat PRGs): nothing reads them
  if (const char *ls = getenv("GMX_RECORD_LINKS"))
    if (atoi(ls) != 0 && !e->dview.is_nested && (rc = set_record_links(e, atoi(ls)))) {
      gmx_engine_destroy(e);
      *out = nullptr;
      return rc;
    }
  // MEASUREMENT HOOK ONLY (profiles/max_candidates: the limit's cost in an unchanged benchmark)
  if (const char *mc = getenv("GMX_MAX_CANDIDATES")) e->max_candidates = (uint32_t)strtoul(mc, nullptr, 10);
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_create")

static int engine_create(const gmx_index *ixh, const gmx_engine_opts *opts_in, gmx_engine *primary, gmx_engine **out) {
  if (!ixh || !out) {
    gmx_set_error("gmx_engine_create: null argument");
    return GMX_EINVAL;
  }
  gmx_engine_opts opts;
  if (opts_in)
    opts = *opts_in;
  else
    gmx_engine_default_opts(&opts);
  if (opts.max_states == 0) opts.max_states = 1024;
  if (opts.max_path_nodes == 0) opts.max_path_nodes = 2048;
  if (opts.max_batch_reads == 0) opts.max_batch_reads = 4u << 20;
  if (opts.huge_heap_bytes == 0) opts.huge_heap_bytes = 512ull << 20;
  if (const char *hb = getenv("GMX_HUGE_HEAP_BYTES")) opts.huge_heap_bytes = strtoull(hb, nullptr, 10);
  opts.huge_heap_bytes = std::max<uint64_t>(opts.huge_heap_bytes, 64 * 1024);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    gmx_set_error("no HIP device available: the quasimap engine has no CPU fallback");
    return GMX_ENODEV;
  }
  if (opts.device < 0 || opts.device >= ndev) {
    gmx_set_error("device ordinal out of range");
    return GMX_ENODEV;
  }
  HIP_TRY(hipSetDevice(opts.device));
  const gmx::HostIndex &h = gmx_index_host(ixh);
  if (h.kmer_size == 0) {
    gmx_set_error("the index was built without a k-mer seed table (kmer_size = 0)");
    return GMX_EINVAL;
  }
  gmx_engine *e = new gmx_engine();
  e->opts = opts;
  GmxIndexView v = h.view();
  int rc = 0;
  {
    std::lock_guard<std::mutex> share_lock(g_dev_index_mu);  // (engines of one group are created side by side: the second waits for the first one's upload)
    GmxDeviceIndex *found = nullptr;
    if (!getenv("GMX_NO_INDEX_SHARE"))
      for (GmxDeviceIndex *d : g_dev_indexes)
        if (d->serial == gmx_index_serial(ixh) && d->device == opts.device) found = d;
    if (found) {
      ++found->refs;
      v = found->view;
      e->index_bytes = found->bytes;
      e->shared_index = found;
    } else {
      rc |= e->upload(&v.blocks, h.blocks);
      rc |= e->upload(&v.hits, h.hits);
      rc |= e->upload(&v.hit_perm, h.hit_perm);
      rc |= e->upload(&v.hit_prog, h.hit_prog);
      rc |= e->upload(&v.text, h.text);
      rc |= e->upload(&v.prog, h.prog);
      rc |= e->upload(&v.sa, h.sa);
      rc |= e->upload(&v.pos_node, h.pos_node);
      rc |= e->upload(&v.nodes, h.nodes);
      rc |= e->upload(&v.edges, h.edges);
      rc |= e->upload(&v.sites, h.sites);
      rc |= e->upload(&v.site_geo, h.site_geo);
      rc |= e->upload(&v.seeds, h.seeds);
      if (h.kmer_size2) rc |= e->upload(&v.seeds2, h.seeds2);
      else v.seeds2 = nullptr;
      rc |= e->upload(&v.seed_words, h.seed_words);
      if (!rc) {  // flags in the multi-state entries of the device copies (GMX_SEEDF_*)
        if (((uint64_t)h.seed_words.size() >> h.seed_shift) >= (1u << 30)) {
          gmx_set_error("the seed tables hold more than 2^30 units of multi-state entries");
          rc = GMX_ECAP;
        } else {
          hipLaunchKernelGGL(gmx_seed_mark_kernel, dim3(4096), dim3(256), 0, nullptr, const_cast<GmxSeed *>(v.seeds), (uint64_t)h.seeds.size(), const_cast<uint32_t *>(v.seed_words), v.seed_shift, v.sa, v.text);
          if (h.kmer_size2)
            hipLaunchKernelGGL(gmx_seed_mark_kernel, dim3(4096), dim3(256), 0, nullptr, const_cast<GmxSeed *>(v.seeds2), (uint64_t)h.seeds2.size(), const_cast<uint32_t *>(v.seed_words), v.seed_shift, v.sa, v.text);
          rc |= hipDeviceSynchronize() != hipSuccess;
        }
      }
      rc |= e->upload(&v.kmer_bitmap, h.kmer_bitmap);

      if (!rc) {  // everything allocated so far is the index: it moves to the shared object
        GmxDeviceIndex *d = new GmxDeviceIndex();
        d->serial = gmx_index_serial(ixh);
        d->device = opts.device;
        d->view = v;
        d->allocs = std::move(e->allocs);
        e->allocs.v.clear();
        d->bytes = e->index_bytes;
        d->refs = 1;
        g_dev_indexes.push_back(d);
        e->shared_index = d;
      }
    }
  }
  e->dview = v;
  e->n_allele = h.n_allele_slots;
  e->n_pb = h.n_pb_slots;
  e->n_grouped = h.n_grouped_slots;
  {  // one contiguous block: a single all-reduce covers the whole coverage (gmx_coverage_device)
    e->n_acc = ((size_t)h.n_acc_slots + 63) / 64 * 64;
    e->n_fused = e->n_acc + 32;
    if (primary)
      e->d_fused = primary->d_fused;  // (the twin records into the engine's accumulators)
    else
      rc |= e->alloc(&e->d_fused, e->n_fused + 32, true);  // + 16 words of read counters + log cursor
    e->d_limbs = e->d_fused ? e->d_fused + e->n_acc : nullptr;
    e->d_stats = e->d_fused ? reinterpret_cast<unsigned long long *>(e->d_fused + e->n_fused) : nullptr;
    e->d_log_cursor = e->d_fused ? e->d_fused + e->n_fused + 16 : nullptr;
    rc |= e->alloc(&e->d_error, 2, true);
    e->phys_allele = h.phys_allele;
    e->phys_pb = h.phys_pb;
    e->phys_grouped = h.phys_grouped;
    e->hit_fix = h.hit_fix;
  }
  // The grouped log is used only by sites with more alleles than get dense group counters (gmx_index.cpp: 8). Between
  // batches the engine looks at its real fill (log_settle): drained when half full; entries that found it full are redone.
  for (const GmxSite &st : h.sites) e->log_sites = e->log_sites || st.grouped_off == GMX_GROUPED_LOG;
  if (!primary && !h.is_nested) {  // what gmx_engine_record_links lays the link block out from (flat PRGs only)
    e->link_alleles.resize(h.sites.size());
    for (size_t s = 0; s < h.sites.size(); ++s) e->link_alleles[s] = (uint8_t)gmx_link_alleles(h.sites[s].n_alleles);
  }
  {  // the lean single-instance coverage kernel where most sites have geometry records (GMX_NO_COVER_JUMP: A/B runs)
    uint64_t n_jump = 0;
    for (const GmxSiteGeo &g : h.site_geo) n_jump += (g.flags & GMX_SITE_JUMP) ? 1u : 0u;
    e->cover_jump = !h.is_nested && 2 * n_jump > h.site_geo.size() && !getenv("GMX_NO_COVER_JUMP");
    // GMX_NO_COVER_JUMP=1 (the escape hatch, and the walk side of tests/test_cover_jump_ab.py): no kernel
    // sees the geometry records, every single-instance read is recorded by the walk as the reference walks it
    if (getenv("GMX_NO_COVER_JUMP")) e->dview.site_geo = nullptr;
  }
  {
    uint64_t cap = opts.log_cap_words ? opts.log_cap_words
                   : e->log_sites     ? (1ull << 26)  // 256 MB; a batch that fills it is settled by drain + replay (log_settle)
                                      : 64;
    e->log_cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFF00ull);
  }
  if (primary)
    e->d_log = primary->d_log;  // (never written: an index with log sites has no twin)
  else
    rc |= e->alloc(&e->d_log, e->log_cap, false);
  e->heap_words = opts.huge_heap_bytes / 4 / 64 * 64;
  rc |= e->alloc(&e->d_heap, e->heap_words, false);
  rc |= e->alloc(&e->d_counters, GMX_N_COUNTERS * GMX_CNT_STRIDE, true);
  // large-capacity pass
  e->ws.big.max_states = opts.max_states;
  e->ws.big.max_path_nodes = opts.max_path_nodes;
  e->ws.big.max_slots = 0;  // its pools are sized with the batch (ensure_batch_capacity)
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, opts.device) == hipSuccess && prop.multiProcessorCount > 0)
      e->n_cus = (uint32_t)prop.multiProcessorCount;
    const size_t words = h.kmer_bitmap.size();
    if (!getenv("GMX_FORCE_ABSENT_FILTER") && words >= 4 && words % 4 == 0 && words * 4 <= 128 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(gmx_filter_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(words * 4)) == hipSuccess)
      e->filter_lds_words = (uint32_t)words;
    (void)hipGetLastError();
    if (primary) {  // (the k-mer filter's tables: the engine's)
      e->filter_lds_words = primary->filter_lds_words;
      e->d_kmer_planar = primary->d_kmer_planar;
      e->d_absent = primary->d_absent;
      e->n_absent = primary->n_absent;
      e->use_absent = primary->use_absent;
    } else if (e->filter_lds_words) {  // re-index the presence bitmap: table index (base j from the left in bit pair j) -> planar
      const uint32_t k = h.kmer_size;
      std::vector<uint32_t> planar(words, 0);
      for (uint64_t code = 0; code < (1ull << (2 * k)); ++code) {
        if (!((h.kmer_bitmap[code >> 5] >> (code & 31)) & 1u)) continue;
        uint32_t lo = 0, hi = 0;
        for (uint32_t j = 0; j < k; ++j) {
          const uint32_t base = (uint32_t)(code >> (2 * j)) & 3u;
          lo |= (base & 1u) << j;
          hi |= (base >> 1) << j;
        }
        const uint32_t p = (hi << k) | lo;
        planar[p >> 5] |= 1u << (p & 31);
      }
      rc |= e->upload(&e->d_kmer_planar, planar);
    } else if (!getenv("GMX_NO_ABSENT_FILTER")) {  // a bitmap too large for LDS: few absent k-mers? (whole-genome PRGs)
      const uint64_t n_k = 1ull << (2 * h.kmer_size);
      if (n_k - std::min<uint64_t>(n_k, h.n_seed_kmers_present) <= GMX_ABSENT_MAX) {
        std::vector<uint32_t> absent;
        for (size_t w = 0; w < words && absent.size() <= GMX_ABSENT_MAX; ++w) {
          uint32_t zeros = ~h.kmer_bitmap[w];
          while (zeros) {
            const uint64_t code = (uint64_t)w * 32 + (uint32_t)__builtin_ctz(zeros);
            zeros &= zeros - 1;
            if (code < n_k) absent.push_back((uint32_t)code);
          }
        }
        if (absent.size() <= GMX_ABSENT_MAX) {
          e->n_absent = (uint32_t)absent.size();
          e->use_absent = true;
          if (absent.empty()) absent.push_back(0);
          rc |= e->upload(&e->d_absent, absent);
        }
      }
    }
  }
  if (const char *pi = getenv("GMX_PROBE_ITERS")) e->probe_iters = (uint32_t)std::max(0, atoi(pi));
  if (getenv("GMX_NO_FUSE")) e->fuse = 0;
  if (const char *eb = getenv("GMX_EXTEND_BUDGET")) e->extend_budget = (uint32_t)std::max(0, atoi(eb));
  e->extend_cap = 0u;  // (GMX_EXTEND_CAP: off by default — at configs[2] a cap of 40 iterations sent 45 k tasks per batch to the
                       //  large-capacity route and the step took 6.4 ms instead of 2.5; see profiles/round4/config2_cap_sweep.txt)
  if (const char *ec = getenv("GMX_EXTEND_CAP")) e->extend_cap = (uint32_t)std::max(0, atoi(ec));
  // passes over the stragglers and the iteration budgets of all but the last. ONE pass by default: at configs[2] (nested
  // MSA regions) three passes — budgets 24 and 96 — take 230 + 528 + 494 us where the single pass takes 901: what is left
  // after the first budget is a few tasks with hundreds of general iterations each (~5 us per iteration: dependent fetches
  // of jump programs and path nodes), and packing them into full waves again does not shorten any of them.
  // GMX_EXTEND_PASSES = "b0,b1": three passes, budgets b0 and b1 (experiments).
  e->extend_passes = 1u;
  e->extend_budget2[0] = 24;
  e->extend_budget2[1] = 96;
  if (const char *ep = getenv("GMX_EXTEND_PASSES")) {
    e->extend_passes = 1;
    for (const char *q = ep; *q && e->extend_passes < GMX_EXTRA_PASSES;) {
      e->extend_budget2[e->extend_passes - 1] = (uint32_t)std::max(1l, strtol(q, const_cast<char **>(&q), 10));
      ++e->extend_passes;
      if (*q == ',') ++q; else break;
    }
  }
  if (getenv("GMX_NO_COOP")) e->coop = false;
  // k-mer entries with many states (small k on a large or dense PRG) do not fit the per-lane stack: when they carry
  // more than 10 % of the seed states the kernels take them one state at a time (seed cursor, a few % slower), else
  // the rare large entry goes to the large-capacity pass
  e->seed_cursor = h.n_seed_states_large * 10 > h.n_seed_states;
  if (const char *sc = getenv("GMX_SEED_CURSOR")) e->seed_cursor = atoi(sc) != 0;
  if (primary) {  // (the twin reads the engine's own copies)
    e->seed_cursor = primary->seed_cursor;
    e->dview.sa_ctx = primary->dview.sa_ctx;
    e->dview.seed_side = primary->dview.seed_side;
  }
  if (!primary && e->seed_cursor && !rc && !getenv("GMX_NO_SA_CTX")) {  // left-context word per suffix-array position (GmxIndexView::sa_ctx): + 4 B per symbol
    uint32_t *sc = nullptr;
    if (e->alloc(&sc, h.sa.size(), false) == GMX_OK) {
      hipLaunchKernelGGL(gmx_sa_ctx_kernel, dim3(8192), dim3(256), 0, nullptr, e->dview.sa, e->dview.text, (uint64_t)h.sa.size(), sc);
      if (hipDeviceSynchronize() == hipSuccess) {
        e->dview.sa_ctx = sc;
        e->index_bytes += h.sa.size() * sizeof(uint32_t);
      }
    } else {
      (void)hipGetLastError();  // (no room: the occurrences are screened through the suffix array and the text, as before)
    }
  }
  // ... and the screening side table of the multi-state entries (GmxIndexView::seed_side; gmx_seed_side_kernel): + a word per
  // four seed words (20 GB at configs[4]). GMX_NO_SEED_SIDE=1: entries are walked header by header as until round 5 (A/B runs).
  if (!primary && e->seed_cursor && !rc && !getenv("GMX_NO_SEED_SIDE") && h.seed_words.size() > 1) {
    uint32_t *side = nullptr;
    const size_t n_side = h.seed_words.size() / 4 + 2;
    if (e->alloc(&side, n_side, false) == GMX_OK) {
      hipLaunchKernelGGL(gmx_seed_side_kernel, dim3(8192), dim3(256), 0, nullptr, e->dview.seeds, (uint64_t)h.seeds.size(), e->dview.seed_words,
                         e->dview.seed_shift, side);
      if (h.kmer_size2)
        hipLaunchKernelGGL(gmx_seed_side_kernel, dim3(8192), dim3(256), 0, nullptr, e->dview.seeds2, (uint64_t)h.seeds2.size(), e->dview.seed_words,
                           e->dview.seed_shift, side);
      if (hipDeviceSynchronize() == hipSuccess) {
        e->dview.seed_side = side;
        e->index_bytes += n_side * sizeof(uint32_t);
      }
    } else {
      (void)hipGetLastError();  // (no room: the screen walks the entries themselves)
    }
  }
  // (stream priorities for the side streams — the few-task kernels first — were measured in round 4: no difference, the
  //  chains there wait for memory, not for wave slots)
  // On a NESTED PRG the twin's streams are created at the HIGHEST stream priority: the runtime keeps a pool of hardware queues per
  // priority (4 each by default), so they get queues of their own. At one priority the engine's and the twin's seven streams share
  // four queues and a twin's main chain sits in a queue behind the engine's straggler kernels: configs[2]'s packed feed 372 M
  // reads/s with one workspace, 436 M with two at one priority, 472 M with the twin's streams on queues of their own
  // (profiles/round6/twin_ab.txt). On a flat PRG every kernel of a batch fills the GPU and precedence for one workspace only
  // delays the other: configs[3] 856 M -> 892 M at one priority, 833 M with the pool. GMX_TWIN_PRIORITY=0 / 1 forces.
  auto make_stream = [&](hipStream_t *st) -> bool {
    int least = 0, greatest = 0;
    bool want_prio = h.is_nested;
    if (const char *tp = getenv("GMX_TWIN_PRIORITY")) want_prio = atoi(tp) != 0;
    const bool prio = primary && want_prio && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest;
    (void)hipGetLastError();
    return (prio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest) : hipStreamCreateWithFlags(st, hipStreamNonBlocking)) == hipSuccess;
  };
  rc |= !make_stream(&e->side_stream);
  rc |= !make_stream(&e->side2_stream);
  rc |= hipEventCreateWithFlags(&e->ev_fork2, hipEventDisableTiming) != hipSuccess;
  rc |= hipEventCreateWithFlags(&e->ev_side1, hipEventDisableTiming) != hipSuccess;
  rc |= hipEventCreateWithFlags(&e->ev_filter, hipEventDisableTiming) != hipSuccess;
  rc |= hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess;
  rc |= hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess;
  e->cover_big_lanes = 64 * 32;
  rc |= e->alloc(&e->d_scratch_big, (size_t)GmxScratchFixed<CoverEnvBig>::total * e->cover_big_lanes, false);
  if (primary) {
    e->is_twin = true;
    rc |= !make_stream(&e->main_stream);
    e->last_stream = e->main_stream;
  }
  if (rc) {
    gmx_engine_destroy(e);
    return GMX_EHIP;
  }
  *out = e;
  return GMX_OK;
}

void gmx_engine_destroy(gmx_engine *e) try {
  if (!e) return;
  (void)hipSetDevice(e->opts.device);
  (void)hipDeviceSynchronize();
  if (e->twin) gmx_engine_destroy(e->twin);
  e->twin = nullptr;
  if (e->main_stream) (void)hipStreamDestroy(e->main_stream);
  if (e->ev_zeroed) (void)hipEventDestroy(e->ev_zeroed);
  if (e->ev_twin_done) (void)hipEventDestroy(e->ev_twin_done);
  if (e->side_stream) (void)hipStreamDestroy(e->side_stream);
  if (e->side2_stream) (void)hipStreamDestroy(e->side2_stream);
  if (e->ev_fork2) (void)hipEventDestroy(e->ev_fork2);
  if (e->ev_side1) (void)hipEventDestroy(e->ev_side1);
  if (e->ev_filter) (void)hipEventDestroy(e->ev_filter);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->ev_wait) (void)hipEventDestroy(e->ev_wait);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->copy_stream2) (void)hipStreamDestroy(e->copy_stream2);
  if (e->h_log_state) (void)hipHostFree(e->h_log_state);
  if (e->ev_log_state) (void)hipEventDestroy(e->ev_log_state);
  for (auto &sl : e->slots) {
    if (sl.copied) (void)hipEventDestroy(sl.copied);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.h_offsets) (void)hipHostFree(sl.h_offsets);
    if (sl.h_seeds) (void)hipHostFree(sl.h_seeds);
  }
  e->ws.allocs.release_all();
  e->allocs.release_all();
  e->outcomes.release();
  e->positions.release();
  gmx_dev_index_release(e->shared_index);
  delete e;
} GMX_GUARD_VOID("gmx_engine_destroy")

int gmx_engine_reset(gmx_engine *e) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  e->reset_pending = false;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(e->d_fused, 0, (e->n_fused + 32) * 4));
  HIP_TRY(hipMemset(e->d_error, 0, 8));
  HIP_TRY(hipMemset(e->d_counters, 0, GMX_N_COUNTERS * GMX_CNT_STRIDE * 4));
  if (e->twin) {
    HIP_TRY(hipMemset(e->twin->d_error, 0, 8));
    HIP_TRY(hipMemset(e->twin->d_counters, 0, GMX_N_COUNTERS * GMX_CNT_STRIDE * 4));
    e->twin_in_flight = false;
  }
  int lrc = e->outcomes.clear(nullptr);
  if (lrc || (lrc = e->positions.clear(nullptr))) return lrc;
  ++e->reset_epoch;
  e->log_counts.clear();
  e->log_known = e->log_reads_since = 0;
  e->log_state_pending = false;
  e->recorded = false;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_reset")

int gmx_engine_reset_async(gmx_engine *e, void *hip_stream) try {
  HIP_TRY(hipSetDevice(e->opts.device));
  hipStream_t st = (hipStream_t)hip_stream;
  int frc = flush_reset(e);  // (an earlier one still pending, on whatever stream it named)
  if (frc) return frc;
  if ((frc = twin_join(e, st))) return frc;  // (the zeroing comes behind whatever the twin still records)
  e->twin_in_flight = false;
  // (the per-read logs: zeroed on the reset's stream now — behind the batches before, ahead of the next one, whose twin launch waits
  //  for the accumulators' zeroing, queued on this stream later; the counts restart with the next launch)
  if ((frc = e->outcomes.clear(&st)) || (frc = e->positions.clear(&st))) return frc;
  ++e->reset_epoch;
  e->reset_pending = true;
  e->reset_stream = st;
  e->log_counts.clear();  // what earlier batches left in the device log goes with the cursor
  e->log_known = e->log_reads_since = 0;
  e->log_state_pending = false;
  e->recorded = false;
  return GMX_OK;
} GMX_GUARD_INT("gmx_engine_reset_async")

}  // extern "C"

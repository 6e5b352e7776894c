// gmx_engine_batch.h — part of gmx_engine.hip's translation unit (gmx_engine_state.h lists the parts): one batch. The workspace's
// growth, a batch as the kernels see it (BatchInput) and its launches on three streams (launch_batch), and the grouped log's
// accounting between batches: drain, settle, replay.
#pragma once
// Grouped log -> host. Waits for the device, adds the log's records to e->log_counts when more than `keep_below` words are in
// use (and empties the device log), and notes how full it is. Records: [site_index, n_ids | strand bit, ids...], each
// worth +1 on its strand (GMX_LOG_REVERSE); GMX_LOG_PAD words are padding (CoverLogPart::log_reserve).
static int log_settle(gmx_engine *e);
static int gmx_log_drain(gmx_engine *e, uint64_t keep_below) {
  int frc = flush_reset(e);
  if (frc) return frc;
  HIP_TRY(hipDeviceSynchronize());
  uint32_t used = 0;
  HIP_TRY(hipMemcpy(&used, e->d_log_cursor, 4, hipMemcpyDeviceToHost));
  used = std::min(used, e->log_cap);
  e->log_reads_since = 0;
  e->log_known = used;
  if (used <= keep_below) return GMX_OK;
  std::vector<uint32_t> w(used);
  HIP_TRY(hipMemcpy(w.data(), e->d_log, (size_t)used * 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> key;
  for (size_t i = 0; i < w.size();) {
    if (w[i] == GMX_LOG_PAD) {
      ++i;
      continue;
    }
    const size_t n_ids = i + 2 > w.size() ? 0 : (size_t)(w[i + 1] & ~GMX_LOG_REVERSE);
    if (i + 2 > w.size() || i + 2 + n_ids > w.size()) {  // reservations are exact (log_reserve): never expected
      gmx_set_error("grouped-allele-count log: malformed record at word " + std::to_string(i) + " of " + std::to_string(w.size()));
      return GMX_EREF;
    }
    if ((w[i + 1] & GMX_LOG_REVERSE) && !(e->owner ? e->owner : e)->record_strands) {  // only CoverAcc::rev_off != 0 sets the bit: never expected
      gmx_set_error("grouped-allele-count log: a reverse-complement record at word " + std::to_string(i) + " of an engine that does not record per strand");
      return GMX_EREF;
    }
    key.assign(1, w[i]);
    key.insert(key.end(), w.begin() + i + 2, w.begin() + i + 2 + n_ids);
    e->log_counts[key][(w[i + 1] & GMX_LOG_REVERSE) ? 1 : 0] += 1;
    i += 2 + n_ids;
  }
  HIP_TRY(hipMemset(e->d_log_cursor, 0, 4));
  e->log_known = 0;
  return GMX_OK;
}

// A coverage instance with its scratch in LDS: one wave per block, as many blocks per CU as scratch copies fit its LDS.
template <class Env, int LIST>
static void launch_cover_lds(gmx_engine *e, hipStream_t stream, const BatchView &b, const SearchOut &o, const CoverAcc &acc,
                             bool after_coop = false) {
  static const uint32_t lanes_env = getenv("GMX_COVER_LANES") ? (uint32_t)atoi(getenv("GMX_COVER_LANES")) : 0u;
  const uint32_t lanes = lanes_env ? std::min(lanes_env, gmx_cover_lds_lanes<Env>()) : gmx_cover_lds_lanes<Env>();
  const size_t lds = (size_t)GmxScratchFixed<Env>::total * lanes * sizeof(uint32_t);
  const uint32_t per_cu = std::min<uint32_t>((uint32_t)(160 * 1024 / lds), 32u);
  hipLaunchKernelGGL((gmx_cover_kernel<Env, LIST>), dim3(e->n_cus * per_cu), dim3(64), lds, stream, e->dview, b, o, e->ws.big,
                     acc, lanes, after_coop ? 1u : 0u, e->links());
}

template <int LIST>
static void launch_cover_coop(gmx_engine *e, hipStream_t stream, const BatchView &b, const SearchOut &o, const CoverAcc &acc) {
  const size_t lds = (size_t)gmx_coop_lds_words<LIST>() * sizeof(uint32_t);
  const uint32_t per_cu = std::min<uint32_t>((uint32_t)(160 * 1024 / lds), 16u);
  hipLaunchKernelGGL((gmx_cover_coop_kernel<LIST>), dim3(e->n_cus * per_cu), dim3(64), lds, stream, e->dview, b, o, e->ws.big, acc, e->links().counts ? 1u : 0u);
}

extern "C" {

// A workspace for launches of up to `cap` reads, built into the empty `w` (which owns whatever was allocated, also on failure)
static int workspace_build(const gmx_engine *e, uint64_t cap, GmxWorkspace &w) {
  const uint64_t n_tasks = cap * 2;
  SearchOut &o = w.o;  // (member by member: the struct's order is not part of any contract)
  GmxAllocs &a = w.allocs;
  int rc;
  if ((rc = a.alloc(&w.d_skip, cap, true))) return rc;
  if ((rc = a.alloc(&o.status, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.n_final, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.cover_recs, n_tasks * GMX_REGIONS, false))) return rc;
  if ((rc = a.alloc(&o.cover_rec_task, n_tasks * GMX_REGIONS, false))) return rc;
  o.region_cap = o.list_stride = o.arena_stride = (uint32_t)n_tasks;
  o.region_inv = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, (((uint64_t)GMX_REGIONS << 32) + e->dview.n_prg - 1) / std::max<uint32_t>(e->dview.n_prg, 1u));
  if ((rc = a.alloc(&o.task_lists, (size_t)GMX_TL_N * n_tasks, false))) return rc;
  o.overflow_list = o.task_lists + (size_t)GMX_TL_OVERFLOW * n_tasks;
  o.overflow2_list = o.task_lists + (size_t)GMX_TL_OVERFLOW2 * n_tasks;
  o.alive_list = o.task_lists + (size_t)GMX_TL_ALIVE * n_tasks;
  o.dead_list = o.task_lists + (size_t)GMX_TL_DEAD * n_tasks;
  o.dead2_list = o.task_lists + (size_t)GMX_TL_DEAD2 * n_tasks;
  o.cover_general_list = o.task_lists + (size_t)GMX_TL_GENERAL * n_tasks;
  if ((rc = a.alloc(&o.cover_overflow_list, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.general_rest_list, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.single_rest_list, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.park2, (size_t)n_tasks * GMX_STACK_DEPTH, false))) return rc;
  if ((rc = a.alloc(&o.park2_n, n_tasks, false))) return rc;
  if (e->log_sites)
    for (int side = 0; side < 2; ++side) {
      if ((rc = a.alloc(&w.log_retry[side], n_tasks, false))) return rc;
      if ((rc = a.alloc(&w.log_retry_recs[side], n_tasks, false))) return rc;
      if ((rc = a.alloc(&w.log_retry_huge[side], n_tasks, false))) return rc;
    }
  if ((rc = a.alloc(&o.cover_mid_list, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.seed_cursor, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.finals, n_tasks * GMX_FAST_STATES, false))) return rc;
  if ((rc = a.alloc(&o.arena, n_tasks * GMX_FAST_ARENA, false))) return rc;
  if ((rc = a.alloc(&o.alive_seed, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.huge_list, n_tasks, false))) return rc;        // the last tier's queues (gmx_tail_stage)
  if ((rc = a.alloc(&o.cover_huge_list, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.huge_retry, 2 * n_tasks, false))) return rc;
  // large-capacity pass: one slot (~60 KB of pools at the default capacities) per task it may have to take; a 1 M-read
  // batch with 5 % of the genome in 10-copy repeats sends 59 k of its 2 M tasks there
  BigOut &big = w.big;
  big.max_states = e->opts.max_states;
  big.max_path_nodes = e->opts.max_path_nodes;
  big.max_slots = (uint32_t)std::min<uint64_t>(n_tasks, std::min<uint64_t>(std::max<uint64_t>(n_tasks / 16, 4096), 262144));
  if ((rc = a.alloc(&big.states, (size_t)big.max_slots * big.max_states, false))) return rc;
  if ((rc = a.alloc(&big.stack, (size_t)big.max_slots * big.max_states * GMX_STACK_WORDS, false))) return rc;
  if ((rc = a.alloc(&big.arena, (size_t)big.max_slots * big.max_path_nodes, false))) return rc;
  if ((rc = a.alloc(&big.n_final, big.max_slots, false))) return rc;
  if ((rc = a.alloc(&big.task_of_slot, big.max_slots, false))) return rc;
  o.slot_n_final = big.n_final;
  o.slot_task = big.task_of_slot;
  if ((rc = a.alloc(&o.big_mapped_list, big.max_slots, false))) return rc;
  o.inst_cap = (uint32_t)std::min<uint64_t>(n_tasks, 1u << 23);  // instance lanes of reads in short repeats (320 B of pools each; gmx_extend_inst_kernel)
  if ((rc = a.alloc(&o.inst_list, o.inst_cap, false))) return rc;
  if ((rc = a.alloc(&o.inst_sa, o.inst_cap, false))) return rc;
  if ((rc = a.alloc(&o.inst_remaining, big.max_slots, false))) return rc;
  if ((rc = a.alloc(&o.inst_mapped_list, big.max_slots, false))) return rc;
  if ((rc = a.alloc(&o.inst_first, big.max_slots, false))) return rc;
  if ((rc = a.alloc(&o.inst_remaining_width, big.max_slots, false))) return rc;
  if ((rc = a.alloc(&o.inst_serial_list, big.max_slots, false))) return rc;  // what gmx_cover_coop_kernel leaves to the serial instances
  if ((rc = a.alloc(&o.general_serial_list, n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.big_serial_list, big.max_slots, false))) return rc;
  if ((rc = a.alloc(&o.overflow3_list, 2 * n_tasks, false))) return rc;
  if ((rc = a.alloc(&o.inst_arena, (size_t)o.inst_cap * GMX_FAST_ARENA, false))) return rc;
  if ((rc = a.alloc(&o.inst_states, (size_t)o.inst_cap * GMX_INST_STATES, false))) return rc;
  w.cap_reads = cap;
  return GMX_OK;
}

// launching: called for a launch of n_reads reads that is about to be enqueued (the reserve calls size the workspace only)
static int ensure_batch_capacity(gmx_engine *e, uint64_t n_reads, bool launching = false) {
  if (launching) {
    gmx_engine *own = e->owner ? e->owner : e;
    for (GmxReadLog *log : {&own->outcomes, &own->positions})
      if (log->on) {
        const int lrc = log->reserve(n_reads);
        if (lrc) return lrc;
      }
  }
  if (n_reads <= e->ws.cap_reads) return GMX_OK;
  // Growth (rare: the first call sizes it): a FRESH workspace, swapped in once all of it exists; the engine is as it was when it
  // does not come about.
  // (an eighth of headroom when the workspace GROWS: chunks of a decoded reads file differ by a few reads — the record a chunk's end
  // cuts — and every growth is two dozen allocations that wait for the device: 11 ms in the middle of `gram`'s second chunk)
  const uint64_t cap = std::max<uint64_t>(e->ws.cap_reads ? n_reads + n_reads / 8 : n_reads, 1024);
  GmxWorkspace fresh;
  fresh.allocs.room(64 + e->ws.allocs.v.size());  // (the bookkeeping of its buffers and of the superseded ones: it may throw only BEFORE there is device memory to lose)
  int rc;
  try {
    rc = workspace_build(e, cap, fresh);
  } catch (...) {
    fresh.allocs.release_all();
    throw;
  }
  if (rc) {  // (nothing enqueued has seen the fresh buffers)
    fresh.allocs.release_all();
    return rc;
  }
  // batches in flight read the superseded buffers: they stay with the workspace's until the engine is destroyed
  fresh.allocs.v.insert(fresh.allocs.v.end(), e->ws.allocs.v.begin(), e->ws.allocs.v.end());
  e->ws.allocs.v.clear();
  std::swap(e->ws, fresh);
  return GMX_OK;
}

static bool gmx_ab_no_filter() {  // A/B runs ONLY (tools/kab.py): no k-mer filter, the two counters it decides stay zero
  static const bool off = getenv("GMX_AB_NO_FILTER") != nullptr;
  return off;
}
static void launch_filter(gmx_engine *e, hipStream_t st, dim3 task_grid, const BatchView &b, const SearchOut &o, int pass,
                          hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr) {
  if (gmx_ab_no_filter()) return;
  if (e->filter_lds_words)
    hipExtLaunchKernelGGL(gmx_filter_lds_kernel, dim3(e->n_cus), dim3(GMX_FILTER_LDS_THREADS), e->filter_lds_words * 4,
                          st, t0, t1, 0u, e->dview, b, o, e->d_kmer_planar, e->filter_lds_words, pass);
  else if (e->use_absent)
    hipExtLaunchKernelGGL(gmx_filter_absent_kernel, task_grid, dim3(GMX_BLOCK), 0, st, t0, t1, 0u, e->dview, b, o, e->d_absent, e->n_absent, pass);
  else
    hipExtLaunchKernelGGL(gmx_filter_kernel, task_grid, dim3(GMX_BLOCK), 0, st, t0, t1, 0u, e->dview, b, o, pass);
}

// ---- grouped log: exact accounting between batches (engines whose index has sites with more than 8 alleles) ----------
static int log_state_enqueue(gmx_engine *e, hipStream_t stream) {
  if (!e->h_log_state) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_log_state), 4 * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_log_state, hipEventDisableTiming));
  }
  HIP_TRY(hipMemcpyAsync(e->h_log_state + 0, e->d_log_cursor, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(e->h_log_state + 1, e->d_counters + GMX_CNT_LOG_RETRY * GMX_CNT_STRIDE, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(e->h_log_state + 2, e->d_counters + GMX_CNT_LOG_RETRY_RECS * GMX_CNT_STRIDE, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(e->h_log_state + 3, e->d_counters + GMX_CNT_LOG_RETRY_HUGE * GMX_CNT_STRIDE, 4, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipEventRecord(e->ev_log_state, stream));
  e->log_state_pending = true;
  return GMX_OK;
}

// The entries of the last batch that found the log full, again: setup (list lengths where the kernels read them), the
// compact records, then the large-scratch coverage instance, whose last block also serves the last tier.
static int launch_log_replay(gmx_engine *e, hipStream_t stream) {
  const int in = e->log_retry_side, out = in ^ 1;
  SearchOut o = e->last_o;
  o.log_retry_list = e->ws.log_retry[out];
  o.log_retry_recs = e->ws.log_retry_recs[out];
  o.log_retry_huge = e->ws.log_retry_huge[out];
  o.cover_overflow_list = e->ws.log_retry[in];  // the queue of gmx_cover_kernel<CoverEnvBig, 1>: this round's entries
  hipLaunchKernelGGL(gmx_log_replay_setup_kernel, dim3(1), dim3(1024), 0, stream, o, e->ws.log_retry_huge[in]);
  if (e->dview.is_nested)
    hipLaunchKernelGGL(gmx_cover_single_replay_kernel<true>, dim3(e->n_cus * 4), dim3(GMX_BLOCK), 0, stream, e->dview, e->last_b, o, e->last_acc,
                     e->ws.log_retry_recs[in]);
  else
    hipLaunchKernelGGL(gmx_cover_single_replay_kernel<false>, dim3(e->n_cus * 4), dim3(GMX_BLOCK), 0, stream, e->dview, e->last_b, o, e->last_acc,
                     e->ws.log_retry_recs[in]);
  hipLaunchKernelGGL((gmx_cover_kernel<CoverEnvBig, 1>), dim3(e->cover_big_lanes / 64), dim3(64), e->last_big_lds, stream, e->dview,
                     e->last_b, o, e->ws.big, e->last_acc, 64u, 0u, e->links());
  HIP_TRY(hipGetLastError());
  e->log_retry_side = out;
  e->last_o.log_retry_list = o.log_retry_list;
  e->last_o.log_retry_recs = o.log_retry_recs;
  e->last_o.log_retry_huge = o.log_retry_huge;
  return log_state_enqueue(e, stream);
}

static int log_settle(gmx_engine *e) {
  if (!e->log_state_pending) return GMX_OK;
  uint64_t before = ~0ull;
  for (int round = 0;; ++round) {
    HIP_TRY(hipEventSynchronize(e->ev_log_state));
    e->log_state_pending = false;
    const uint32_t used = std::min(e->h_log_state[0], e->log_cap);
    const uint64_t retries = (uint64_t)e->h_log_state[1] + e->h_log_state[2] + e->h_log_state[3];
    if (retries == 0) {
      if (used > e->log_cap / 2) return gmx_log_drain(e, 0);
      e->log_known = used;
      return GMX_OK;
    }
    if (round > 0 && retries >= before) {  // (every round starts with an empty log: each must get at least one entry through)
      // an emptied log did not hold one task's records: only more memory helps (gmx_engine_sync reports the read)
      HIP_TRY(hipDeviceSynchronize());
      const uint32_t err[2] = {GMX_TASK_LOGFULL, 0};
      HIP_TRY(hipMemcpy(e->d_error, err, 8, hipMemcpyHostToDevice));
      return GMX_OK;
    }
    before = retries;
    int rc = gmx_log_drain(e, 0);
    if (rc) return rc;
    e->log_replays++;
    e->log_replayed_entries += retries;
    if ((rc = launch_log_replay(e, e->last_stream))) return rc;
  }
}

// One batch as the kernels see it: reads as bytes (d_reads + d_offsets: gmx_pack_kernel makes the bit planes) or as bit
// planes already (d_planes; gmx_map_reads_packed_host).
struct BatchInput {
  const uint8_t *d_reads = nullptr;
  const uint64_t *d_offsets = nullptr;  // null with uniform_len
  const uint32_t *d_seeds = nullptr;
  const uint2 *d_planes = nullptr;      // non-null: packed input, no pack kernel
  const uint8_t *d_skip = nullptr;      // packed input: per-read skip flags, or null
  const uint32_t *d_twobit = nullptr;   // non-null: the reads as a 2-bit stream (gmx_map_reads_2bit_host); unpacked into d_packed
  uint32_t twobit_base0 = 0;            // ... whose first base sits at this base index of d_twobit (< 32)
  uint32_t uniform_len = 0;
  uint64_t n_reads = 0, total_bases = 0;
};

// first kernel of a batch whose reads arrive packed: what gmx_pack_kernel does besides packing (queue counters, a queued reset)
__global__ void gmx_batch_begin_kernel(uint32_t *counters, uint32_t *zero, uint32_t zero_words) {
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < GMX_N_COUNTERS * GMX_CNT_STRIDE; i += blockDim.x) counters[i] = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < zero_words; i += gridDim.x * blockDim.x) zero[i] = 0;
}

// Reads that arrive as a 2-bit stream (include/gmx.h, gmx_pack_reads_2bit: base j of the batch in bits 2j, 2j + 1) -> the bit
// planes the kernels read, in gmx_pack_kernel's layout. One thread per pair of planes (32 bases): three words of the
// stream, funnel-shifted to the pair's first base, even bits -> low plane, odd bits -> high plane.
__device__ __forceinline__ uint32_t gmx_even_bits(unsigned long long x) {  // bits 0, 2, 4, .. 62 of x, compacted
  x &= 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)x;
}
__global__ void __launch_bounds__(256) gmx_unpack2_kernel(BatchView b, const uint32_t *stream, uint32_t base0, uint2 *packed) {
  const uint32_t ppr_uniform = b.pairs_per_read;
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;; t += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t read, pair;
    uint64_t first_base;  // of the read, in the batch's stream
    uint32_t len;
    if (b.uniform_len) {
      read = (uint32_t)(t / ppr_uniform);
      if (read >= b.n_reads) break;
      pair = (uint32_t)(t - (uint64_t)read * ppr_uniform);
      first_base = (uint64_t)read * b.uniform_len;
      len = b.uniform_len;
    } else {  // ragged: one thread per read walks its pairs (the plane layout needs the offsets anyway)
      read = (uint32_t)t;
      if (read >= b.n_reads) break;
      pair = 0;
      first_base = b.offsets[read] - b.offsets[0];
      len = (uint32_t)(b.offsets[read + 1] - b.offsets[read]);
    }
    uint2 *out = packed + pack_off(b, read);
    const uint32_t n_pairs = b.uniform_len ? pair + 1 : (len + 31u) / 32u;
    for (uint32_t p = pair; p < n_pairs; ++p) {
      const uint64_t j = base0 + first_base + 32ull * p;  // base index in the stream of the pair's first base
      const uint64_t w = j >> 4;                         // 16 bases per word
      const uint32_t sh = (uint32_t)(j & 15u) * 2u;
      const uint32_t w0 = stream[w], w1 = stream[w + 1], w2 = stream[w + 2];
      const unsigned long long bits = (unsigned long long)__builtin_amdgcn_alignbit(w1, w0, sh) |
                                      ((unsigned long long)__builtin_amdgcn_alignbit(w2, w1, sh) << 32);
      out[p] = make_uint2(gmx_even_bits(bits), gmx_even_bits(bits >> 1));
    }
  }
}

static int launch_batch(gmx_engine *e, const BatchInput &in, hipStream_t stream) {
  const uint64_t n_reads = in.n_reads, total_bases = in.total_bases;
  if (n_reads == 0) return GMX_OK;
  if (n_reads > (0x7fffffffull / GMX_FAST_ARENA) / 2) {  // path-node handles (offsets into the arena table) stay below 2^31
    gmx_set_error("batch too large: at most 44 M reads per launch (lower gmx_engine_opts.max_batch_reads)");
    return GMX_EINVAL;
  }
  // the batch before: redo what found the log full, drain when half full. FIRST: a replay reads that batch's queues and
  // retry lists, which a growing workspace (ensure_batch_capacity) replaces with fresh, uninitialised buffers.
  int rc = e->log_sites ? log_settle(e) : GMX_OK;
  if (rc) return rc;
  if ((rc = ensure_batch_capacity(e, n_reads, true))) return rc;
  const bool fold_reset = e->reset_pending && e->reset_stream == stream;
  if (e->reset_pending && !fold_reset && (rc = flush_reset(e))) return rc;
  e->reset_pending = false;
  if (!in.d_planes) {
    const uint64_t need = total_bases / 32 + n_reads + 16;  // pairs; the slack covers the one-pair look-ahead of planes()
    if ((rc = e->grow(e->packed, need, need, 0, true))) return rc;  // (the batches before read the planes they were given: those stay)
  }
  BatchView b{in.d_reads, in.d_offsets, in.d_seeds, (in.d_planes || in.d_twobit) ? in.d_skip : e->ws.d_skip, in.d_planes ? in.d_planes : e->packed.d,
              (uint32_t)n_reads, (uint32_t)(e->opts.forward_only ? 1 : 0), in.uniform_len, (in.uniform_len + 31u) / 32u,
              e->keep_states ? 1u : 0u};
  SearchOut o = e->ws.o;  // every per-batch pointer and capacity; what belongs to the launch:
  o.error = e->d_error;
  o.counters = e->d_counters;
  o.stats = e->d_stats;
  o.inst_slots = !getenv("GMX_NO_INST") ? e->ws.big.max_slots : 0u;
  o.split_twice = getenv("GMX_NO_SPLIT2") ? 0u : 1u;
  o.log_retry_list = e->ws.log_retry[e->log_retry_side];
  o.log_retry_recs = e->ws.log_retry_recs[e->log_retry_side];
  o.log_retry_huge = e->ws.log_retry_huge[e->log_retry_side];
  {
    gmx_engine *own = e->owner ? e->owner : e;
    own->recorded = true;
    if (own->outcomes.on) {  // (room was made in ensure_batch_capacity)
      o.outcomes = own->outcomes.d;
      o.outcome_base = own->outcomes.claim(n_reads);
    }
    if (own->positions.on) {
      o.positions = reinterpret_cast<uint2 *>(own->positions.d);
      o.position_base = own->positions.claim(n_reads);
    }
  }
  uint32_t n_tasks = (uint32_t)n_reads * 2;
  if (e->keep_states) {  // test hook: a task that never reaches a kernel that writes its state count reads as "no state"
    HIP_TRY(hipMemsetAsync(o.n_final, 0, (size_t)n_tasks * sizeof(uint32_t), stream));
    e->keep_reads = n_reads;
  }
  gmx_engine::EvTriple ev{};
  if (e->timing) {
    HIP_TRY(hipEventCreate(&ev.s));
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    HIP_TRY(hipEventCreate(&ev.c));
    for (int k = 0; k < GMX_TK_N; ++k) {
      HIP_TRY(hipEventCreate(&ev.k[k][0]));
      HIP_TRY(hipEventCreate(&ev.k[k][1]));
    }
    ev.reads = n_reads;
    HIP_TRY(hipEventRecord(ev.s, stream));
  }
  // (timing leg: events attached to the dispatches themselves — their own start and end, as a kernel trace sees them)
  auto t_ev = [&](int k, int side) -> hipEvent_t {
    if (!e->timing) return nullptr;
    ev.timed |= 1u << k;
    return ev.k[k][side];
  };
  if (in.d_planes || in.d_twobit) {
    hipLaunchKernelGGL(gmx_batch_begin_kernel, dim3(fold_reset ? 256 : 1), dim3(1024), 0, stream, e->d_counters,
                       fold_reset ? e->d_fused : nullptr, fold_reset ? (uint32_t)(e->n_fused + 32) : 0u);
    if (in.d_twobit) {
      const uint64_t threads = in.uniform_len ? n_reads * ((in.uniform_len + 31u) / 32u) : n_reads;
      hipExtLaunchKernelGGL(gmx_unpack2_kernel, dim3((unsigned)std::min<uint64_t>((threads + 255) / 256, 1u << 20)), dim3(256), 0, stream,
                            t_ev(GMX_TK_UNPACK, 0), t_ev(GMX_TK_UNPACK, 1), 0u, b, in.d_twobit, in.twobit_base0, e->packed.d);
    }
  } else
    hipLaunchKernelGGL(gmx_pack_kernel, dim3((unsigned)((n_reads + GMX_PACK_READS - 1) / GMX_PACK_READS)), dim3(GMX_PACK_THREADS), 0, stream, b,
                       e->ws.d_skip, e->packed.d, e->d_counters, fold_reset ? e->d_fused : nullptr, fold_reset ? (uint32_t)(e->n_fused + 32) : 0u);
  if (fold_reset && (rc = note_zeroed(e, stream))) return rc;  // (the batch's first kernel zeroed the accumulators: the twin's next batch waits for it)
  size_t lds = (size_t)GMX_STACK_DEPTH * GMX_STACK_WORDS * GMX_BLOCK * sizeof(uint32_t);
  const size_t big_lds = (size_t)GMX_BIG_LDS_DEPTH * GMX_STACK_WORDS * 64 * sizeof(uint32_t);
  dim3 task_grid((n_tasks + GMX_BLOCK - 1) / GMX_BLOCK);
  const bool seeded = e->dview.kmer_size2 != 0 && !getenv("GMX_NO_SEEDED");  // longer seed table: no probe phase (gmx_seed_kernel)
  if (seeded)
    hipExtLaunchKernelGGL(gmx_seed_kernel, dim3((n_tasks + GMX_SEED_THREADS * GMX_SEED_CHUNKS - 1) / (GMX_SEED_THREADS * GMX_SEED_CHUNKS)), dim3(GMX_SEED_THREADS), 0, stream,
                          t_ev(GMX_TK_SEED, 0), t_ev(GMX_TK_SEED, 1), 0u, e->dview, b, o);
  else if (e->seed_cursor)
    hipExtLaunchKernelGGL(gmx_probe_kernel<true>, task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, t_ev(GMX_TK_SEED, 0), t_ev(GMX_TK_SEED, 1), 0u, e->dview, b, o,
                          e->probe_iters);
  else
    hipExtLaunchKernelGGL(gmx_probe_kernel<false>, task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, t_ev(GMX_TK_SEED, 0), t_ev(GMX_TK_SEED, 1), 0u, e->dview, b, o,
                          e->probe_iters);
  // fork 1: the probe kernel's overflow queue (few, long-running tasks) is served by the large-capacity kernel on a
  // side stream while the extend kernel runs, and so is the k-mer filter of the tasks the probe kernel found dead
  // (most reverse-complement tasks; the extend kernel queues its own dead tasks separately)
  HIP_TRY(hipEventRecord(e->ev_fork, stream));
  HIP_TRY(hipStreamWaitEvent(e->side_stream, e->ev_fork, 0));
  CoverAcc acc{e->d_fused, e->d_log, e->d_log_cursor, e->log_cap, e->d_scratch_big, e->cover_big_lanes, e->opts.rng_mode,
               (e->owner ? e->owner : e)->max_candidates, e->log_sites ? 1u : 0u, e->d_heap, e->heap_words, o.status, (uint32_t)n_reads * 2u, e->d_stats,
               (e->owner ? e->owner : e)->record_strands ? (uint32_t)e->n_acc : 0u, (uint32_t)e->tally_off()};
  if (seeded) {  // what gmx_seed_kernel sent to the large-capacity pass (reads in repeats), and its coverage: on side 2
    HIP_TRY(hipStreamWaitEvent(e->side2_stream, e->ev_fork, 0));
    const InstPools pools{0};
    // one lane per mapping instance of the reads in short repeats, then their coverage. (On a stream of its own this pair
    // gained nothing: the runtime then put two of the four streams on one hardware queue, and filter and extend kernel
    // ran one after the other.)
    hipLaunchKernelGGL(gmx_extend_inst_kernel, dim3(e->n_cus * 2), dim3(GMX_BLOCK), lds, e->side2_stream, e->dview, b, o, pools);
    if (e->coop) launch_cover_coop<5>(e, e->side2_stream, b, o, acc);
    launch_cover_lds<CoverEnvMid, 5>(e, e->side2_stream, b, o, acc, e->coop);
    hipLaunchKernelGGL(gmx_search_split_kernel, dim3(4096), dim3(64), big_lds, e->side2_stream, e->dview, b, o, e->ws.big, 0);
    launch_cover_lds<CoverEnvMid, 4>(e, e->side2_stream, b, o, acc);
  } else {
    hipLaunchKernelGGL(gmx_search_big_kernel, dim3(1024), dim3(64), big_lds, e->side_stream, e->dview, b, o, e->ws.big, 0);
  }
  HIP_TRY(hipEventRecord(e->ev_side1, e->side_stream));
  if (!gmx_ab_no_filter()) launch_filter(e, e->side_stream, task_grid, b, o, 0, t_ev(GMX_TK_FILTER0, 0), t_ev(GMX_TK_FILTER0, 1));
  // (timing leg: the events are attached to this very dispatch — its own start and end, as a kernel trace sees them —
  // instead of being recorded around it, where they add the gap to the kernel before and two barrier packets)
  hipEvent_t k0 = e->timing ? ev.a : nullptr, k1 = e->timing ? ev.b : nullptr;
  const uint32_t budget = e->extend_budget;
  if (seeded && e->seed_cursor)
    hipExtLaunchKernelGGL((gmx_extend_kernel<true, 1>), task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, k0, k1, 0u, e->dview, b, o, e->fuse, budget, 0u);
  else if (seeded)
    hipExtLaunchKernelGGL((gmx_extend_kernel<false, 1>), task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, k0, k1, 0u, e->dview, b, o, e->fuse, budget, 0u);
  else if (e->seed_cursor)
    hipExtLaunchKernelGGL((gmx_extend_kernel<true, 0>), task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, k0, k1, 0u, e->dview, b, o, e->fuse, budget, 0u);
  else
    hipExtLaunchKernelGGL((gmx_extend_kernel<false, 0>), task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, k0, k1, 0u, e->dview, b, o, e->fuse, budget, 0u);
  if (budget) {  // the stragglers, compacted (a block that finds its part of the queue empty returns at once)
    for (uint32_t pass = 0; pass < e->extend_passes; ++pass) {
      const bool last = pass + 1 >= e->extend_passes;
      // (the last pass runs to the end, or — nested PRGs — to its cap, beyond which a task goes to the split search)
      const uint32_t budget2 = last ? e->extend_cap : e->extend_budget2[pass];
      const uint32_t pass_arg = pass | (last && e->extend_cap ? 0x80000000u : 0u);
      hipEvent_t p0 = pass == 0 ? t_ev(GMX_TK_EXTEND2, 0) : nullptr, p1 = pass == 0 ? t_ev(GMX_TK_EXTEND2, 1) : nullptr;
      if (e->seed_cursor)
        hipExtLaunchKernelGGL((gmx_extend_kernel<true, 2>), task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, p0, p1, 0u, e->dview, b, o, e->fuse, budget2, pass_arg);
      else
        hipExtLaunchKernelGGL((gmx_extend_kernel<false, 2>), task_grid, dim3(GMX_BLOCK), (uint32_t)lds, stream, p0, p1, 0u, e->dview, b, o, e->fuse, budget2, pass_arg);
    }
  }
  // fork 2: the extend kernel's overflow queue, then the coverage of everything the large-capacity kernel mapped,
  // beside filter + coverage of the regular tasks
  HIP_TRY(hipEventRecord(e->ev_fork2, stream));
  HIP_TRY(hipStreamWaitEvent(e->side2_stream, e->ev_fork2, 0));
  HIP_TRY(hipStreamWaitEvent(e->side2_stream, e->ev_side1, 0));
  // the second filter pass (the tasks the extend kernel found dead) comes first here: side 1 is busy with the first pass
  // for most of the batch, and behind the few-lane kernels below it would end after the main stream's last kernel
  if (!gmx_ab_no_filter()) launch_filter(e, e->side2_stream, task_grid, b, o, 1, t_ev(GMX_TK_FILTER1, 0), t_ev(GMX_TK_FILTER1, 1));
  // the extend kernel's overflow queue (and the tasks whose instances ran out of their pools): the 16-lane split search
  // first, one lane with a whole slot for what that leaves
  static const bool split2 = getenv("GMX_NO_SPLIT2") == nullptr;
  if (split2) hipLaunchKernelGGL(gmx_search_split_kernel, dim3(1024), dim3(64), big_lds, e->side2_stream, e->dview, b, o, e->ws.big, 1);
  hipLaunchKernelGGL(gmx_search_big_kernel, dim3(1024), dim3(64), big_lds, e->side2_stream, e->dview, b, o, e->ws.big, split2 ? 2 : 1);
  if (e->coop) launch_cover_coop<2>(e, e->side2_stream, b, o, acc);
  launch_cover_lds<CoverEnvMid, 2>(e, e->side2_stream, b, o, acc, e->coop);
  // the general instances of the regular tasks: their queue is complete after the extend kernel unless the PRG is
  // nested (there gmx_cover_single_kernel hands tasks over), so they run on side 1, off the main stream (and not behind
  // the large-capacity pass's chain of few-lane kernels: with reads in repeats that chain is the batch's longest path)
  const bool general_on_side = !e->dview.is_nested;
  HIP_TRY(hipStreamWaitEvent(e->side_stream, e->ev_fork2, 0));
  // links between nearby sites (gmx_engine_record_links): the region queues are complete behind the extend kernel's last pass —
  // one lane per compact record on side 1, beside the single-instance kernel on the main stream; joined through ev_filter below
  if (const GmxLinks lk = e->links(); lk.counts)
    hipLaunchKernelGGL(gmx_link_kernel, dim3(task_grid.x * GMX_REGIONS), dim3(GMX_BLOCK), 0, e->side_stream, e->dview, o, lk);
  const size_t one_lds = (size_t)4 * GMX_WIDE_LOCI * GMX_ONE_THREADS * sizeof(uint32_t);
  const bool one = !getenv("GMX_NO_COVER_ONE");
  auto launch_one = [&](hipStream_t st) {  // (with GMX_NO_COVER_ONE the kernel only passes its queue on: A/B runs)
    hipLaunchKernelGGL(gmx_cover_one_kernel, dim3(e->n_cus * 4), dim3(GMX_ONE_THREADS), one_lds, st, e->dview, b, o, e->ws.big, acc, one ? 1u : 0u, e->links().counts ? 1u : 0u);
  };
  if (general_on_side) {
    launch_one(e->side_stream);
    if (e->coop) launch_cover_coop<3>(e, e->side_stream, b, o, acc);
    launch_cover_lds<CoverEnvLds, 3>(e, e->side_stream, b, o, acc, e->coop);
    launch_cover_lds<CoverEnv, 0>(e, e->side_stream, b, o, acc);
  }
  HIP_TRY(hipEventRecord(e->ev_filter, e->side_stream));
  // (Round 4 measured the records in PRG order — a radix sort of (position, record) pairs in front of this kernel, for the
  //  locality of the accumulator and table lines: at configs[3] the kernel took 508 us instead of 436 plus 120 us of sorting, at
  //  configs[4] 646 instead of 611: neighbouring lanes then hit the SAME accumulator words and their atomics serialise. Dropped.)
  if (e->dview.is_nested) {
    hipExtLaunchKernelGGL(gmx_cover_single_kernel<true>, dim3(task_grid.x * GMX_REGIONS), dim3(GMX_BLOCK), 0, stream, t_ev(GMX_TK_SINGLE, 0), t_ev(GMX_TK_SINGLE, 1), 0u,
                          e->dview, b, o, acc);
  } else if (e->cover_jump) {  // most sites have geometry records: the lean kernel, then the few records it declined
    // (Measured and dropped: this kernel over the records queued by then BESIDE the extend kernel's passes over the stragglers,
    //  those moved to side 1 — at configs[3] the passes then took 335 us instead of 165 and the batch 1.13 ms instead of 1.07:
    //  the two kernels wait for the same thing, the memory system's rate of scattered accesses.)
    hipExtLaunchKernelGGL(gmx_cover_jump_kernel, dim3(task_grid.x * GMX_REGIONS), dim3(GMX_BLOCK), (uint32_t)(GMX_STAGE_MAX * GMX_BLOCK * sizeof(uint32_t)), stream,
                          t_ev(GMX_TK_SINGLE, 0), t_ev(GMX_TK_SINGLE, 1), 0u, e->dview, b, o, acc);
    hipLaunchKernelGGL(gmx_cover_single_rest_kernel, dim3(e->n_cus * 2), dim3(GMX_BLOCK), 0, stream, e->dview, b, o, acc);
  } else {
    hipExtLaunchKernelGGL(gmx_cover_single_kernel<false>, dim3(task_grid.x * GMX_REGIONS), dim3(GMX_BLOCK), 0, stream, t_ev(GMX_TK_SINGLE, 0), t_ev(GMX_TK_SINGLE, 1), 0u,
                          e->dview, b, o, acc);
  }
  // The batch's last coverage instance (1: what exceeded the regular scratch; its last block also serves the last tier,
  // whose search keeps its first pending entries in LDS) needs every other instance done except gmx_cover_single_kernel,
  // which queues nothing on a non-nested PRG: there it runs at the end of side 2, beside that kernel.
  hipStream_t last = general_on_side ? e->side2_stream : stream;
  if (!general_on_side) {
    launch_one(stream);
    if (e->coop) launch_cover_coop<3>(e, stream, b, o, acc);
    launch_cover_lds<CoverEnvLds, 3>(e, stream, b, o, acc, e->coop);
    launch_cover_lds<CoverEnv, 0>(e, stream, b, o, acc);
    HIP_TRY(hipEventRecord(e->ev_join, e->side2_stream));
    HIP_TRY(hipStreamWaitEvent(stream, e->ev_join, 0));
  }
  HIP_TRY(hipStreamWaitEvent(last, e->ev_filter, 0));
  hipLaunchKernelGGL((gmx_cover_kernel<CoverEnvBig, 1>), dim3(e->cover_big_lanes / 64), dim3(64), big_lds, last, e->dview,
                     b, o, e->ws.big, acc, 64u, 0u, e->links());
  if (general_on_side) {
    HIP_TRY(hipEventRecord(e->ev_join, e->side2_stream));
    HIP_TRY(hipStreamWaitEvent(stream, e->ev_join, 0));
  }
  // (no pass over per-task status words: the read counters are added where each task's fate is decided, SearchOut::stats)
  if (e->timing) {
    HIP_TRY(hipEventRecord(ev.c, stream));
    e->pending.push_back(ev);
  }
  HIP_TRY(hipGetLastError());
  e->last_stream = stream;
  if (e->log_sites) {  // what log_settle() looks at before the next batch, and what a replay needs of this one
    e->last_b = b;
    e->last_o = o;
    e->last_acc = acc;
    e->last_big_lds = big_lds;
    if ((rc = log_state_enqueue(e, stream))) return rc;
  }
  return GMX_OK;
}

}  // extern "C"

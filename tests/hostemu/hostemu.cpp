// hostemu.cpp — TEST-ONLY host build of the per-lane device logic (gmx_core.h + gmx_cover.h).
//
// The HIP kernels in gramtools_amd/csrc/gmx_engine.hip run these headers one lane per task. There is no
// GPU in the build container, so this file drives the SAME headers sequentially on the host with the same
// capacities, letting `-m "not gpu"` tests check the search/selection/recording logic against the oracle
// before GPU time is spent. It is never linked into libgmx.so and the product never loads it.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

// which routine recorded a single-instance task on a flat PRG (gmx_cover_single): 0 walk-free, 1 jump, 2 the walk
static uint64_t g_cover_routes[3];
#define GMX_COVER_ROUTE(k) (++g_cover_routes[k])
static uint32_t g_stage_cap = 0;  // hostemu_set_stage: operations gmx_cover_jump may stage (0: it records in a second pass)
#define GMX_COVER_TEST_STAGE g_stage_cap
#include "../../gramtools_amd/csrc/gmx_core.h"
#include "../../gramtools_amd/csrc/gmx_cover.h"
#include "../../gramtools_amd/csrc/gmx_dfs.h"
#include "../../gramtools_amd/csrc/gmx_index.h"

namespace {

struct EmuCtx {
  std::vector<GmxFinalState> st;
  uint32_t n = 0, cap;
  std::vector<GmxPathNode> arena;
  uint32_t arena_cap;
  uint32_t status = GMX_TASK_MAPPED;
  EmuCtx(uint32_t c, uint32_t ac) : st(c), cap(c), arena_cap(ac) {}
  uint32_t n_states() const { return n; }
  void set_n_states(uint32_t v) { n = v; }
  void get(uint32_t s, uint32_t &lo, uint32_t &hi, uint32_t &tvd, uint32_t &tvg) const {
    lo = st[s].lo; hi = st[s].hi; tvd = st[s].traversed; tvg = st[s].traversing;
  }
  void put(uint32_t s, uint32_t lo, uint32_t hi, uint32_t tvd, uint32_t tvg) { st[s] = GmxFinalState{lo, hi, tvd, tvg}; }
  bool push(uint32_t lo, uint32_t hi, uint32_t tvd, uint32_t tvg) {
    if (n >= cap) return false;
    put(n++, lo, hi, tvd, tvg);
    return true;
  }
  uint32_t arena_new(uint32_t site, int32_t allele, uint32_t next) {
    if (arena.size() >= arena_cap) return GMX_NIL;
    arena.push_back(GmxPathNode{site, allele, next});
    return (uint32_t)arena.size() - 1;
  }
  uint32_t arena_site(uint32_t node) const { return arena[node].site; }
  uint32_t arena_next(uint32_t node) const { return arena[node].next; }
  void fail(uint32_t s) {
    if (status == GMX_TASK_MAPPED || s == GMX_TASK_ERROR) status = s;
  }
};

// Mirror of FastCtx in gmx_engine.hip: bounded LIFO of pending entries, bounded emit buffer, inline traversing handle.
struct EmuDfsCtx {
  struct Entry {
    uint32_t a, b, tvd, tvg, pos, mode;
  };
  std::vector<Entry> stack;
  uint32_t stack_cap;
  std::vector<GmxFinalState> out;
  uint32_t out_cap;
  std::vector<GmxPathNode> arena;
  uint32_t arena_cap;
  uint32_t status = GMX_TASK_MAPPED;
  EmuDfsCtx(uint32_t sc, uint32_t oc, uint32_t ac) : stack_cap(sc), out_cap(oc), arena_cap(ac) {}
  bool pop(uint32_t &a, uint32_t &b, uint32_t &tvd, uint32_t &tvg, uint32_t &pos, uint32_t &mode) {
    if (stack.empty()) return false;
    Entry e = stack.back();
    stack.pop_back();
    a = e.a; b = e.b; tvd = e.tvd; tvg = e.tvg; pos = e.pos; mode = e.mode;
    return true;
  }
  bool push(uint32_t a, uint32_t b, uint32_t tvd, uint32_t tvg, uint32_t pos, uint32_t mode) {
    if (stack.size() >= stack_cap) return false;
    stack.push_back(Entry{a, b, tvd, tvg, pos, mode});
    return true;
  }
  bool emit(uint32_t lo, uint32_t hi, uint32_t tvd, uint32_t tvg) {
    if (out.size() >= out_cap) return false;
    out.push_back(GmxFinalState{lo, hi, tvd, tvg});
    return true;
  }
  uint32_t alloc_node(uint32_t site, int32_t allele, uint32_t next) {
    if (arena.size() >= arena_cap) return GMX_NIL;
    arena.push_back(GmxPathNode{site, allele, next});
    return (uint32_t)arena.size() - 1;
  }
  uint32_t arena_new(uint32_t site, int32_t allele, uint32_t next) {
    if (allele == -1) {
      if (next == GMX_NIL) return GMX_INLINE_FLAG | ((site - 5u) >> 1);
      if (gmx_h_inline(next)) {
        next = alloc_node(gmx_h_site(arena.data(), next), -1, GMX_NIL);
        if (next == GMX_NIL) return GMX_NIL;
      }
    }
    return alloc_node(site, allele, next);
  }
  uint32_t arena_site(uint32_t h) const { return gmx_h_site(arena.data(), h); }
  uint32_t arena_next(uint32_t h) const { return gmx_h_next(arena.data(), h); }
  void fail(uint32_t s) {
    if (status == GMX_TASK_MAPPED || s == GMX_TASK_ERROR) status = s;
  }
};

struct Emu {
  gmx::HostIndex h;
  std::vector<uint32_t> acc, log;  // the accumulator block (gmx_types.h) as on the device
  uint64_t stats[5] = {0, 0, 0, 0, 0};
  int rng_mode = 0;
  uint32_t first_error = 0, error_task = 0;
  uint64_t n_overflow_tasks = 0, n_cover_overflow = 0, n_cover_huge = 0;
  // one count per hand-over of the coverage ladder (hostemu_sizes [7..]): Lds -> CoverEnv, CoverEnv -> Big, Mid -> Big, tasks the
  // general routine saw (fast pass / large-capacity search), tasks the cooperative instances 3 / 2 / 5 would reject (hostemu_set_coop)
  uint64_t n_lds_to_regular = 0, n_regular_to_big = 0, n_mid_to_big = 0, n_general_fast = 0, n_general_big = 0, n_coop_reject_fast = 0,
           n_coop_reject_big = 0, n_coop5_reject_big = 0;
  uint32_t seed_split = 0;  // hostemu_set_seed_split: gmx_seed_kernel's rule (GMX_SEED_SPLIT_MAX; 0: off)
  Emu *dry = nullptr;  // (takes the dry run's records, never read)
  int coop = 0;  // hostemu_set_coop: state the cooperative instances' reject rule per task (costs a dry run of the routine)
  uint32_t single_loci = GMX_SINGLE_LOCI;  // hostemu_set_single_loci: force the nested single-instance routine to give up
  int wide = 0;  // hostemu_set_wide: single-instance tasks take gmx_cover_single_nested_wide first (gmx_cover_one_kernel's routine)
  uint64_t n_wide = 0;
  std::string err;
};

template <uint32_t I_, uint32_t B_, uint32_t LOC_, uint32_t H_, uint32_t P_ = GMX_PATH_CACHE>
struct EmuEnvT {
  static constexpr uint32_t I_MAX = I_, B_MAX = B_, LOC_MAX = LOC_, H_MAX = H_, P_MAX = P_;
  static constexpr uint32_t i_max() { return I_; }
  static constexpr uint32_t b_max() { return B_; }
  static constexpr uint32_t loc_max() { return LOC_; }
  static constexpr uint32_t h_max() { return H_; }
  bool has_log_sites() const { return true; }
  bool log_reserve(uint32_t words) {
    reserved += words;
    return true;
  }
  uint32_t reserved = 0, appended = 0;  // the reservation must cover exactly what the task appends
  std::vector<uint32_t> scratch;
  const GmxPathNode *arena;
  uint32_t h_site(uint32_t h) const { return gmx_h_site(arena, h); }
  int32_t h_allele(uint32_t h) const { return gmx_h_allele(arena, h); }
  uint32_t h_next(uint32_t h) const { return gmx_h_next(arena, h); }
  Emu *e;
  uint32_t status = GMX_TASK_MAPPED;
  EmuEnvT() : scratch(GmxScratchFixed<EmuEnvT>::total, 0xDEADBEEFu) {}
  uint32_t sget(uint32_t w) const { return scratch.at(w); }
  void sset(uint32_t w, uint32_t v) { scratch.at(w) = v; }
  uint32_t single_loci() const { return e->single_loci; }
  void add_allele_sum(uint32_t s) { e->acc.at(s)++; }
  void add_per_base(uint32_t s) { e->acc.at(s)++; }
  void add_hit(uint32_t s) { e->acc.at(s)++; }
  void add_grouped_dense(uint32_t s) { e->acc.at(s)++; }
  void add_allele_and_group(uint32_t s) {
    e->acc.at(s)++;
    e->acc.at(s + 1)++;
  }
  bool log_grouped_begin(uint32_t site, uint32_t n) {
    e->log.push_back(site);
    e->log.push_back(n);
    appended += 2;
    return true;
  }
  void log_grouped_id(int32_t a) {
    e->log.push_back((uint32_t)a);
    ++appended;
  }
  void log_grouped_end() {}
  void fail(uint32_t s) {
    if (status == GMX_TASK_MAPPED || s == GMX_TASK_ERROR) status = s;
  }
};

// Mirror of CoverEnvDyn (gmx_engine.hip): the last tier, capacities decided per task.
struct EmuEnvDyn {
  uint32_t cap_i, cap_b, cap_loc, cap_h;
  uint32_t i_max() const { return cap_i; }
  uint32_t b_max() const { return cap_b; }
  uint32_t loc_max() const { return cap_loc; }
  uint32_t h_max() const { return cap_h; }
  bool has_log_sites() const { return true; }
  bool log_reserve(uint32_t words) {
    reserved += words;
    return true;
  }
  uint32_t reserved = 0, appended = 0;
  std::vector<uint32_t> scratch;
  const GmxPathNode *arena;
  uint32_t h_site(uint32_t h) const { return gmx_h_site(arena, h); }
  int32_t h_allele(uint32_t h) const { return gmx_h_allele(arena, h); }
  uint32_t h_next(uint32_t h) const { return gmx_h_next(arena, h); }
  Emu *e;
  uint32_t status = GMX_TASK_MAPPED;
  uint32_t sget(uint32_t w) const { return scratch.at(w); }
  void sset(uint32_t w, uint32_t v) { scratch.at(w) = v; }
  uint32_t single_loci() const { return e->single_loci; }
  void add_allele_sum(uint32_t s) { e->acc.at(s)++; }
  void add_per_base(uint32_t s) { e->acc.at(s)++; }
  void add_hit(uint32_t s) { e->acc.at(s)++; }
  void add_grouped_dense(uint32_t s) { e->acc.at(s)++; }
  void add_allele_and_group(uint32_t s) {
    e->acc.at(s)++;
    e->acc.at(s + 1)++;
  }
  bool log_grouped_begin(uint32_t site, uint32_t n) {
    e->log.push_back(site);
    e->log.push_back(n);
    appended += 2;
    return true;
  }
  void log_grouped_id(int32_t a) {
    e->log.push_back((uint32_t)a);
    ++appended;
  }
  void log_grouped_end() {}
  void fail(uint32_t s) {
    if (status == GMX_TASK_MAPPED || s == GMX_TASK_ERROR) status = s;
  }
};

// The engine's fixed tiers (gmx_engine_cover_kernels.h), from the same statement of their capacities (gmx_cover.h)
typedef EmuEnvT<GMX_TIER_ARGS(GMX_CAPS_LDS)> EmuEnvLds;      // CoverEnvLds
typedef EmuEnvT<GMX_TIER_ARGS(GMX_CAPS_MID)> EmuEnvMid;      // CoverEnvMid
typedef EmuEnvT<GMX_TIER_ARGS(GMX_CAPS_REGULAR)> EmuEnv;     // CoverEnv
typedef EmuEnvT<GMX_TIER_ARGS(GMX_CAPS_BIG)> EmuEnvBig;      // CoverEnvBig
// The host has no wave: the cooperative instances are mirrored as their reject rule alone (coop_rejects). An item lane's
// scratch, and the rest of the rule as one scratch for gmx_cover_task: up to 16 items, keys and path cache of an item lane,
// loci and hull of the class scratch.
template <int LIST>
struct EmuCoop {
  typedef EmuEnvT<GMX_TIER_ARGS(GMX_CAPS_COOP_ITEM)> Item;
  typedef EmuEnvT<GMX_COOP_UNITS, GMX_CAPS_COOP_ITEM.key_sites, GMX_CAPS_COOP_CLASS.loci, GMX_CAPS_COOP_CLASS.hull, GMX_CAPS_COOP_ITEM.path> Task;
};
template <>
struct EmuCoop<5> {
  typedef EmuEnvT<GMX_TIER_ARGS(GMX_CAPS_COOP5_ITEM)> Item;
  typedef EmuEnvT<GMX_COOP_UNITS, GMX_CAPS_COOP5_ITEM.key_sites, GMX_CAPS_COOP5_CLASS.loci, GMX_CAPS_COOP5_CLASS.hull, GMX_CAPS_COOP5_ITEM.path> Task;
};

struct Read {
  const uint8_t *p;
  uint32_t len;
  bool rc;
  uint32_t at(uint32_t i) const { return rc ? 5u - p[len - 1 - i] : p[i]; }
  // bit planes of raw bases start .. start + 31 (what the pack kernel's output gives the device reader)
  void planes(uint32_t start, uint32_t &lo, uint32_t &hi) const {
    lo = hi = 0;
    for (uint32_t j = 0; j < 32 && start + j < len; ++j) {
      uint32_t code = p[start + j] - 1u;
      lo |= (code & 1u) << j;
      hi |= ((code >> 1) & 1u) << j;
    }
  }
};

uint32_t kmer_code(const Read &r, uint32_t start, uint32_t k) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < k; ++j) c |= (r.at(start + j) - 1u) << (2 * j);  // table index: rightmost base most significant (gmx_types.h)
  return c;
}

bool all_kmers_present(const GmxIndexView &ix, const Read &r) {
  uint32_t k = ix.kmer_size;
  for (uint32_t o = 0; o + k <= r.len; ++o) {
    uint32_t code = kmer_code(r, o, k);
    if (!((ix.kmer_bitmap[code >> 5] >> (code & 31)) & 1u)) return false;
  }
  return true;
}

void load_seed(const GmxIndexView &ix, uint32_t code, EmuCtx &ctx) {
  GmxSeed s = ix.seeds[code];
  if (s.a != GMX_SEED_COMPLEX) {
    if (s.a <= s.b) ctx.push(s.a, s.b, GMX_NIL, GMX_NIL);
    return;
  }
  const uint32_t *p = ix.seed_words + ((size_t)s.b << ix.seed_shift);
  uint32_t ns = *p++;
  for (uint32_t i = 0; i < ns; ++i) {
    uint32_t lo = p[0], hi = p[1], nt = p[2], ng = p[3];
    p += 4;
    uint32_t tvd = GMX_NIL, tvg = GMX_NIL;
    bool ok = true;
    for (uint32_t j = 0; j < nt; ++j, p += 2) {
      if (!ok) continue;
      uint32_t nn = ctx.arena_new(p[0], (int32_t)p[1], tvd);
      if (nn == GMX_NIL) ok = false; else tvd = nn;
    }
    for (uint32_t j = 0; j < ng; ++j, ++p) {
      if (!ok) continue;
      uint32_t nn = ctx.arena_new(p[0], -1, tvg);
      if (nn == GMX_NIL) ok = false; else tvg = nn;
    }
    if (!ok || !ctx.push(lo, hi, tvd, tvg)) {
      ctx.fail(GMX_TASK_OVERFLOW);
      return;
    }
  }
}

// probe (GMX_PROBE_STEPS bases, survivors parked) + extend, as gmx_probe_kernel / gmx_extend_kernel do
void dfs_task(const GmxIndexView &ix, const Read &r, EmuDfsCtx &ctx, uint32_t probe_steps, uint32_t final_cap) {
  const uint32_t k = ix.kmer_size;
  const uint32_t from = r.len - k;
  const uint32_t stop = from > probe_steps ? from - probe_steps : 0;
  GmxSeed s = ix.seeds[kmer_code(r, from, k)];
  if (s.a != GMX_SEED_COMPLEX) {
    if (s.a <= s.b) ctx.push(s.a, s.b, GMX_NIL, GMX_NIL, from, GMX_MODE_STATE);
  } else {
    const uint32_t *p = ix.seed_words + ((size_t)s.b << ix.seed_shift);
    uint32_t ns = *p++;
    for (uint32_t i = 0; i < ns; ++i) {
      uint32_t lo = p[0], hi = p[1], nt = p[2], ng = p[3];
      p += 4;
      uint32_t tvd = GMX_NIL, tvg = GMX_NIL;
      bool ok = true;
      for (uint32_t j = 0; j < nt; ++j, p += 2) {
        if (!ok) continue;
        uint32_t nn = ctx.arena_new(p[0], (int32_t)p[1], tvd);
        if (nn == GMX_NIL) ok = false; else tvd = nn;
      }
      for (uint32_t j = 0; j < ng; ++j, ++p) {
        if (!ok) continue;
        uint32_t nn = ctx.arena_new(p[0], -1, tvg);
        if (nn == GMX_NIL) ok = false; else tvg = nn;
      }
      if (!ok || !ctx.push(lo, hi, tvd, tvg, from, GMX_MODE_STATE)) {
        ctx.fail(GMX_TASK_OVERFLOW);
        return;
      }
    }
  }
  if (ctx.status != GMX_TASK_MAPPED) return;
  Read rr = r;
  gmx_dfs_run(ix, ctx, rr, stop);
  if (ctx.status != GMX_TASK_MAPPED || stop == 0 || ctx.out.empty()) return;
  // extend phase: parked states go back on the stack, finals replace them
  std::vector<GmxFinalState> parked;
  parked.swap(ctx.out);
  ctx.out_cap = final_cap;
  for (auto &f : parked) ctx.push(f.lo, f.hi, f.traversed, f.traversing, stop, GMX_MODE_STATE);
  gmx_dfs_run(ix, ctx, rr, 0);
}

void search_task(const GmxIndexView &ix, const Read &r, EmuCtx &ctx) {
  uint32_t k = ix.kmer_size;
  load_seed(ix, kmer_code(r, r.len - k, k), ctx);
  if (ctx.status != GMX_TASK_MAPPED) return;
  for (uint32_t i = r.len - k; i-- > 0;) {
    if (ctx.n_states() == 0) break;
    gmx_extend(ix, r.at(i), ctx);
    if (ctx.status != GMX_TASK_MAPPED) return;
  }
}

// gmx_cover_coop_kernel's reject rule for one task: more than 16 final states or units (a path-bearing or text-form state is
// one unit, a pathless interval one per occurrence), an item that exceeds an item lane's scratch, or a drawn class that
// exceeds the class scratch. `dry` takes the dry run's records and is never read.
template <int LIST>
bool coop_rejects(const GmxIndexView &ix, Emu *dry, const GmxFinalState *st, uint32_t nf, const GmxPathNode *arena, uint32_t len,
                  uint32_t seed, int rng_mode) {
  if (nf > GMX_COOP_UNITS) return true;
  uint64_t units = 0;
  for (uint32_t f = 0; f < nf; ++f)
    units += (st[f].traversed != GMX_NIL || st[f].traversing != GMX_NIL || gmx_text_form(st[f].hi)) ? 1u : (uint64_t)(st[f].hi - st[f].lo) + 1u;
  if (units > GMX_COOP_UNITS) return true;
  typedef typename EmuCoop<LIST>::Item ItemEnv;
  typedef GmxScratch<ItemEnv> SI;
  bool over = false;
  gmx_final_items(ix, st, nf,
                  [&](uint32_t lo, uint32_t hi, uint32_t tvd, uint32_t tvg, uint32_t es, int32_t ea) -> bool {
                    ItemEnv ie;  // the lane's own scratch: one item, its loci window and key
                    ie.e = dry;
                    ie.arena = arena;
                    const uint32_t w[6] = {lo, hi, tvd, tvg, es, (uint32_t)ea};
                    for (uint32_t t = 0; t < 6; ++t) ie.sset(SI::items + t, w[t]);
                    const uint32_t nl = gmx_item_loci(ix, ie, 0, 0);
                    if (nl != 0xFFFFFFFFu) gmx_item_key(ix, ie, 0, 0, nl);
                    over = over || ie.status == GMX_TASK_OVERFLOW;
                    return true;
                  },
                  [](uint32_t, uint32_t) {});
  if (over) return true;
  typename EmuCoop<LIST>::Task te;  // the drawn class against the class scratch
  te.e = dry;
  te.arena = arena;
  gmx_cover_task(ix, te, st, nf, len, seed, rng_mode);
  return te.status == GMX_TASK_OVERFLOW;
}

// One fixed tier: gmx_cover_task with that tier's scratch. -> the task's status (a log reservation that does not cover what
// the task appended is an error)
template <class Env>
uint32_t cover_with(const GmxIndexView &ix, Emu *e, const GmxFinalState *st, uint32_t nf, const GmxPathNode *arena, uint32_t len,
                    uint32_t seed) {
  Env env;
  env.arena = arena;
  env.e = e;
  gmx_cover_task(ix, env, st, nf, len, seed, e->rng_mode);
  if (env.status == GMX_TASK_MAPPED && env.reserved != env.appended) return GMX_TASK_ERROR;
  return env.status;
}

}  // namespace

extern "C" {

void *hostemu_create(const uint32_t *prg, uint64_t n, uint32_t k, int rng_mode, char *err, uint64_t errcap) {
  try {
    Emu *e = new Emu();
    gmx::build_index(std::vector<uint32_t>(prg, prg + n), k, e->h, 1);
    e->acc.assign(e->h.n_acc_slots, 0);
    e->rng_mode = rng_mode;
    return e;
  } catch (std::exception const &ex) {
    if (err && errcap) {
      strncpy(err, ex.what(), errcap - 1);
      err[errcap - 1] = 0;
    }
    return nullptr;
  }
}
void hostemu_destroy(void *p) {
  delete ((Emu *)p)->dry;
  delete (Emu *)p;
}
void hostemu_set_seed_split(void *p, uint32_t n) { static_cast<Emu *>(p)->seed_split = n; }
void hostemu_set_coop(void *p, int on) {
  Emu *e = static_cast<Emu *>(p);
  e->coop = on;
  if (on && !e->dry) {
    e->dry = new Emu();
    e->dry->acc.assign(e->acc.size(), 0);
  }
}
// The fixed tiers' capacities as the headers state them, five words each (GmxTierCaps): Lds, Mid, CoverEnv, Big, the
// cooperative Item and Class of instances 3 / 2, those of instance 5; then GMX_COOP_UNITS, GMX_SINGLE_LOCI, GMX_WIDE_LOCI.
void hostemu_capacities(uint32_t *out) {
  const GmxTierCaps all[8] = {GMX_CAPS_LDS, GMX_CAPS_MID, GMX_CAPS_REGULAR, GMX_CAPS_BIG, GMX_CAPS_COOP_ITEM, GMX_CAPS_COOP_CLASS,
                              GMX_CAPS_COOP5_ITEM, GMX_CAPS_COOP5_CLASS};
  for (int t = 0; t < 8; ++t) {
    const uint32_t w[5] = {all[t].items, all[t].key_sites, all[t].loci, all[t].hull, all[t].path};
    for (int i = 0; i < 5; ++i) out[5 * t + i] = w[i];
  }
  out[40] = GMX_COOP_UNITS;
  out[41] = GMX_SINGLE_LOCI;
  out[42] = GMX_WIDE_LOCI;
}

// Same two-tier flow as launch_batch(): fast pass, large-capacity pass, the coverage ladder, stats.
void hostemu_set_wide(void *p, int on) { static_cast<Emu *>(p)->wide = on; }
void hostemu_routes(uint64_t *out, int reset) {
  for (int i = 0; i < 3; ++i) {
    out[i] = g_cover_routes[i];
    if (reset) g_cover_routes[i] = 0;
  }
}
void hostemu_set_stage(uint32_t cap) { g_stage_cap = cap; }
uint64_t hostemu_n_wide(void *p) { return static_cast<Emu *>(p)->n_wide; }
void hostemu_set_single_loci(void *p, uint32_t n) { static_cast<Emu *>(p)->single_loci = n < GMX_SINGLE_LOCI ? n : GMX_SINGLE_LOCI; }

int hostemu_map(void *p, const uint8_t *reads, const uint64_t *offsets, const uint32_t *seeds, uint64_t n_reads,
                uint32_t fast_states, uint32_t fast_arena, uint32_t big_states, uint32_t big_arena) {
  Emu *e = (Emu *)p;
  GmxIndexView ix = e->h.view();
  for (uint64_t read = 0; read < n_reads; ++read) {
    uint32_t len = (uint32_t)(offsets[read + 1] - offsets[read]);
    bool bad = false;
    for (uint32_t i = 0; i < len; ++i) {
      uint8_t v = reads[offsets[read] + i];
      if (v < 1 || v > 4) bad = true;
    }
    for (int o = 0; o < 2; ++o) {
      e->stats[0]++;
      if (bad || len < ix.kmer_size || len == 0) {
        e->stats[1]++;
        continue;
      }
      Read r{reads + offsets[read], len, o == 1};
      // fast tier: the DFS loop with the kernel's capacities (stack = fast_states - 2, parked <= stack, finals <= fast_states)
      EmuDfsCtx dfs(fast_states > 2 ? fast_states - 2 : 1, fast_states > 2 ? fast_states - 2 : 1, fast_arena);
      // gmx_seed_kernel: a path-less seed over more positions than the fast pass takes apart goes straight to the searches behind it
      const GmxSeed sd = ix.seeds[kmer_code(r, len - ix.kmer_size, ix.kmer_size)];
      bool seed_over = e->seed_split && sd.a != GMX_SEED_COMPLEX && sd.a <= sd.b && sd.b - sd.a >= e->seed_split;
      if (e->seed_split && sd.a == GMX_SEED_COMPLEX) {  // (gmx_seed_mark_kernel: a multi-state entry with such a path-less state)
        const uint32_t *w = ix.seed_words + ((size_t)sd.b << ix.seed_shift);
        const uint32_t ns = *w++;
        for (uint32_t j = 0; j < ns; ++j) {
          seed_over = seed_over || (w[1] >= w[0] + e->seed_split && w[2] == 0 && w[3] == 0);
          w += 4 + 2 * w[2] + w[3];
        }
      }
      if (seed_over)
        dfs.status = GMX_TASK_OVERFLOW;
      else
        dfs_task(ix, r, dfs, 6, fast_states);
      EmuCtx big(big_states, big_arena);
      struct View {
        const GmxFinalState *st;
        uint32_t n;
        const GmxPathNode *arena;
        uint32_t status;
      } use{dfs.out.data(), (uint32_t)dfs.out.size(), dfs.arena.data(), dfs.status};
      if (dfs.status == GMX_TASK_OVERFLOW) {
        e->n_overflow_tasks++;
        search_task(ix, r, big);
        use = View{big.st.data(), big.n, big.arena.data(), big.status};
      }
      if (use.status != GMX_TASK_MAPPED) {
        if (!e->first_error) {
          e->first_error = use.status;
          e->error_task = (uint32_t)(read * 2 + o);
        }
        continue;
      }
      if (use.n == 0) {
        if (all_kmers_present(ix, r)) e->stats[3]++; else e->stats[2]++;
        continue;
      }
      e->stats[4]++;
      const bool from_big = use.st == big.st.data();  // a task of the large-capacity search
      uint32_t cstatus = GMX_TASK_MAPPED;
      bool taken = false;
      if (e->wide && use.n == 1 && (gmx_text_form(use.st[0].hi) || use.st[0].lo == use.st[0].hi)) {
        EmuEnv env;
        env.arena = use.arena;
        env.e = e;
        taken = gmx_cover_single_nested_wide(ix, env, use.st[0], len);  // false: nothing recorded, the general routine next
        if (taken) e->n_wide++;
        if (taken) cstatus = env.status == GMX_TASK_MAPPED && env.reserved != env.appended ? GMX_TASK_ERROR : env.status;
      }
      if (!taken) {
        // The ladder of gmx_engine_batch.h. An entry that exceeds a scratch has recorded nothing yet: the next tier redoes it.
        //   fast pass:              CoverEnvLds -> CoverEnv -> CoverEnvBig -> the heap-backed tier
        //   large-capacity search:  CoverEnvMid -> CoverEnvBig -> the heap-backed tier
        (from_big ? e->n_general_big : e->n_general_fast)++;
        if (e->coop) {
          Emu &dry = *e->dry;
          const bool rej = from_big ? coop_rejects<2>(ix, &dry, use.st, use.n, use.arena, len, seeds[read], e->rng_mode)
                                    : coop_rejects<3>(ix, &dry, use.st, use.n, use.arena, len, seeds[read], e->rng_mode);
          if (rej) (from_big ? e->n_coop_reject_big : e->n_coop_reject_fast)++;
          // (instance 5 takes the same kind of task when the engine searched it one lane per instance: its smaller scratch)
          if (from_big && coop_rejects<5>(ix, &dry, use.st, use.n, use.arena, len, seeds[read], e->rng_mode)) e->n_coop5_reject_big++;
          dry.log.clear();
        }
        if (from_big) {
          cstatus = cover_with<EmuEnvMid>(ix, e, use.st, use.n, use.arena, len, seeds[read]);
          if (cstatus == GMX_TASK_OVERFLOW) e->n_mid_to_big++;
        } else {
          cstatus = cover_with<EmuEnvLds>(ix, e, use.st, use.n, use.arena, len, seeds[read]);
          if (cstatus == GMX_TASK_OVERFLOW) {
            e->n_lds_to_regular++;
            cstatus = cover_with<EmuEnv>(ix, e, use.st, use.n, use.arena, len, seeds[read]);
            if (cstatus == GMX_TASK_OVERFLOW) e->n_regular_to_big++;
          }
        }
      }
      if (cstatus == GMX_TASK_OVERFLOW) {  // the large scratch
        e->n_cover_overflow++;
        cstatus = cover_with<EmuEnvBig>(ix, e, use.st, use.n, use.arena, len, seeds[read]);
      }
      if (cstatus == GMX_TASK_OVERFLOW) {  // the last tier (gmx_tail_item): scratch sized for this task
        e->n_cover_huge++;
        EmuEnvDyn dyn;
        uint32_t n_items = 0;
        for (uint32_t f = 0; f < use.n; ++f) {
          const GmxFinalState &st = use.st[f];
          if (st.traversed != GMX_NIL || st.traversing != GMX_NIL) {
            ++n_items;
            continue;
          }
          for (uint32_t i = st.lo;; ++i) {
            n_items += ix.nodes[ix.pos_node[gmx_occ_pos(ix, st.hi, i)]].site != 0;
            if (gmx_text_form(st.hi) || i == st.hi) break;
          }
        }
        dyn.cap_i = n_items ? n_items : 1;
        dyn.cap_b = len + 8 > 32 ? len + 8 : 32;
        dyn.cap_loc = dyn.cap_h = 1u << 16;
        dyn.scratch.assign(GmxScratch<EmuEnvDyn>::total_of(dyn), 0xDEADBEEFu);
        dyn.arena = use.arena;
        dyn.e = e;
        gmx_cover_task(ix, dyn, use.st, use.n, len, seeds[read], e->rng_mode);
        cstatus = dyn.status;
        if (cstatus == GMX_TASK_MAPPED && dyn.reserved != dyn.appended) cstatus = GMX_TASK_ERROR;
      }
      if (cstatus != GMX_TASK_MAPPED && !e->first_error) {
        e->first_error = cstatus;
        e->error_task = (uint32_t)(read * 2 + o);
      }
    }
  }
  return e->first_error ? -(int)e->first_error : 0;
}

void hostemu_sizes(void *p, uint64_t *out) {
  Emu *e = (Emu *)p;
  out[0] = e->h.n_allele_slots;
  out[1] = e->h.n_pb_slots;
  out[2] = e->h.n_grouped_slots;
  out[3] = e->log.size();
  out[4] = e->n_overflow_tasks;
  out[5] = e->n_cover_overflow;
  out[6] = e->n_cover_huge;
  // one count per hand-over ([5] = [8] + [9])
  out[7] = e->n_lds_to_regular;
  out[8] = e->n_regular_to_big;
  out[9] = e->n_mid_to_big;
  out[10] = e->n_general_fast;
  out[11] = e->n_general_big;
  out[12] = e->n_coop_reject_fast;
  out[13] = e->n_coop_reject_big;
  out[14] = e->n_coop5_reject_big;
}
void hostemu_fetch(void *p, uint32_t *allele_sum, uint32_t *per_base, uint32_t *grouped, uint32_t *log, uint64_t *stats) {
  Emu *e = (Emu *)p;
  for (size_t i = 0; i < e->h.phys_allele.size(); ++i) allele_sum[i] = e->acc[e->h.phys_allele[i]];
  for (size_t i = 0; i < e->h.phys_pb.size(); ++i) per_base[i] = e->acc[e->h.phys_pb[i]];
  for (size_t i = 0; i < e->h.phys_grouped.size(); ++i) grouped[i] = e->acc[e->h.phys_grouped[i]];
  for (size_t i = 0; i + 3 < e->h.hit_fix.size(); i += 4) {
    const uint32_t hits = e->acc[e->h.hit_fix[i]];
    allele_sum[e->h.hit_fix[i + 1]] += hits;
    grouped[e->h.hit_fix[i + 2]] += hits;
    per_base[e->h.hit_fix[i + 3]] += hits;
  }
  if (!e->log.empty()) memcpy(log, e->log.data(), e->log.size() * 4);
  memcpy(stats, e->stats, sizeof(e->stats));
}

}  // extern "C"

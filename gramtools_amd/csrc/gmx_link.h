// gmx_link.h — allele pairs seen on one read: links between nearby sites (gmx_engine_record_links).
//
// A task (read, orientation) that is exactly mapped with ONE mapping instance has one path: the allele it starts inside, if
// any, and the (site, allele) loci it traverses, ascending by site on a flat PRG. For every two of its loci i < j whose site
// indices lie at most `span` apart it adds 1 to M(s_i, s_j - s_i)[a_i][a_j]. Only sites with at most GMX_LINK_MAX_ALLELES
// alleles take part ("linkable": the limit of the dense group counters); A'(s) is the allele count of a linkable site, 0 of
// any other site and past the last one.
//
// Layout of the counters (a function of the index and the span alone):
//   off[0] = 0, off[s + 1] - off[s] = A'(s) * sum_{d = 1..span} A'(s + d)
//   M(s, d) starts at off[s] + A'(s) * sum_{e = 1..d-1} A'(s + e) and is row-major [allele at s][allele at s + d]
// The device reads one 8-byte word per locus (GmxLinkSite): the site's offset and A' of the site and of its next seven sites,
// four bits each. Everything a pair needs of its LEFT locus is in that locus's word; of the right one only site and allele.
//
// The one routine below serves gmx_link_kernel (compact records: CompactEnv's handles) and gmx_cover_task's single-instance
// shortcut (arena handles), on the device and in host builds. It needs nothing of Env but h_site / h_allele / h_next.
#pragma once
#include "gmx_types.h"

#define GMX_LINK_MAX_SPAN 7u
#define GMX_LINK_MAX_ALLELES 8u
#ifndef GMX_LINK_BATCH
#define GMX_LINK_BATCH 4u  // per-site words fetched side by side (independent loads: the reason GMX_JUMP_BATCH gives)
#endif

GMX_HD uint32_t gmx_link_alleles(uint32_t n_alleles) { return n_alleles <= GMX_LINK_MAX_ALLELES ? n_alleles : 0u; }

struct GmxLinkSite {
  uint32_t off;      // off[s]: the first word of the site's matrices in the link block
  uint32_t alleles;  // bits 4e .. 4e+3: A'(s + e), e = 0 .. 7
};

struct GmxLinks {
  const GmxLinkSite *site;  // one word per site of the engine's site index
  uint32_t *counts;         // the link block; nullptr: off
  uint32_t span;            // 1 .. GMX_LINK_MAX_SPAN
  uint32_t n_sites;
  GMX_HD void add(uint32_t word) const {
#if defined(__HIP_DEVICE_COMPILE__)
    // (atomicAdd's builtin — relaxed, device scope, the value not used: fire and forget — so that host translation units that
    //  hipcc also compiles for the device need no runtime header for this file)
    (void)__hip_atomic_fetch_add(&counts[word], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    counts[word] += 1u;
#endif
  }
};

// off[0 .. n_sites] of the layout above; alleles(s) is the site's allele count (any number: gmx_link_alleles is applied here)
template <class Alleles>
inline void gmx_link_offsets(uint64_t n_sites, uint32_t span, Alleles alleles, uint64_t *off) {
  off[0] = 0;
  for (uint64_t s = 0; s < n_sites; ++s) {
    uint64_t right = 0;
    for (uint64_t d = 1; d <= span && s + d < n_sites; ++d) right += gmx_link_alleles(alleles(s + d));
    off[s + 1] = off[s] + (uint64_t)gmx_link_alleles(alleles(s)) * right;
  }
}

// The pairs of one single-instance task. p: the PRG position of the read's first base; tvd / tvg: the traversed list (ascending by
// site) and the traversing handle of its one state. A task with fewer than two loci returns before any load of this feature.
template <class Env>
GMX_HD void gmx_link_path(const GmxLinks &lk, const GmxIndexView &ix, const Env &env, uint32_t p, uint32_t tvd, uint32_t tvg) {
  if (tvd == GMX_NIL) return;                                // at most the allele the read starts inside
  if (tvg == GMX_NIL && env.h_next(tvd) == GMX_NIL) return;  // one locus
  // the last loci as a shift register (static indices only: registers, not scratch memory); [0] is the newest
  uint32_t rs[GMX_LINK_MAX_SPAN] = {}, ro[GMX_LINK_MAX_SPAN] = {}, rf[GMX_LINK_MAX_SPAN] = {}, ra[GMX_LINK_MAX_SPAN] = {}, n_ring = 0;
  auto push = [&](const uint32_t s, const GmxLinkSite w, const uint32_t allele) {
    const uint32_t aj = allele < 15u ? allele : 15u;  // (15 and more: beyond every linkable site's alleles, adds nothing)
#pragma unroll
    for (uint32_t k = 0; k < GMX_LINK_MAX_SPAN; ++k) {
      if (k >= n_ring) continue;
      const uint32_t d = s - rs[k];
      if (d - 1u >= lk.span) continue;  // (d = 0 and a list that is not ascending wrap to "too far")
      const uint32_t f = rf[k], a_left = f & 15u, a_right = (f >> (4u * d)) & 15u;  // A'(s_i), A'(s_i + d) = A'(s_j)
      if (ra[k] >= a_left || aj >= a_right) continue;  // a non-linkable end (A' = 0) or an allele out of range
      uint32_t between = (f >> 4) & ((1u << (4u * (d - 1u))) - 1u);  // A'(s_i + 1) .. A'(s_i + d - 1): their sum
      between = (between & 0x0F0F0F0Fu) + ((between >> 4) & 0x0F0F0F0Fu);
      between = (between * 0x01010101u) >> 24;
      lk.add(ro[k] + a_left * between + ra[k] * a_right + aj);
    }
#pragma unroll
    for (uint32_t k = GMX_LINK_MAX_SPAN - 1u; k > 0; --k) rs[k] = rs[k - 1u], ro[k] = ro[k - 1u], rf[k] = rf[k - 1u], ra[k] = ra[k - 1u];
    rs[0] = s, ro[0] = w.off, rf[0] = w.alleles, ra[0] = aj;
    n_ring = n_ring < GMX_LINK_MAX_SPAN ? n_ring + 1u : n_ring;
  };
  uint32_t x = tvd;
  bool lead = tvg != GMX_NIL;  // the allele the read starts inside: the locus in front of the list, in the first batch
  do {
    uint32_t m = 0, s[GMX_LINK_BATCH] = {}, a[GMX_LINK_BATCH] = {};
    GmxLinkSite w[GMX_LINK_BATCH] = {};
#pragma unroll
    for (uint32_t j = 0; j < GMX_LINK_BATCH; ++j) {
      if (j == 0 && lead) {
        s[0] = (env.h_site(tvg) - 5u) >> 1;
        a[0] = 0xFFFFFFFFu;
        m = 1;
      } else if (x != GMX_NIL) {
        s[j] = (env.h_site(x) - 5u) >> 1;
        a[j] = (uint32_t)env.h_allele(x);
        x = env.h_next(x);
        m = j + 1u;
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < GMX_LINK_BATCH; ++j)
      if (j < m) w[j] = s[j] < lk.n_sites ? lk.site[s[j]] : GmxLinkSite{0u, 0u};
    if (lead) a[0] = (uint32_t)ix.nodes[ix.pos_node[p]].allele;  // (behind the batch's words: a chain of two dependent loads)
    lead = false;
#pragma unroll
    for (uint32_t j = 0; j < GMX_LINK_BATCH; ++j)
      if (j < m) push(s[j], w[j], a[j]);
  } while (x != GMX_NIL);
}

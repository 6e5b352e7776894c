// Host check of gmx_link_path and gmx_link_offsets (gramtools_amd/csrc/gmx_link.h): hand-built paths over a small table of sites,
// against the pairs of DESIGN §6.6 written out directly. Stand-alone (its own main), so it can be built with sanitizers:
// tests/test_site_links_host.py compiles it with -fsanitize=address,undefined and runs it. Prints "ok <checks>" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "gmx_link.h"

struct ListEnv {  // a path as arena nodes; an inline handle is the traversing site (gmx_types.h)
  std::vector<GmxPathNode> arena;
  uint32_t h_site(uint32_t h) const { return gmx_h_site(arena.data(), h); }
  int32_t h_allele(uint32_t h) const { return gmx_h_allele(arena.data(), h); }
  uint32_t h_next(uint32_t h) const { return gmx_h_next(arena.data(), h); }
};

static const uint32_t kAlleles[] = {2, 3, 4, 2, 9, 3, 2, 4, 8, 2, 3, 2, 2, 16, 2};  // a 9-allele and a 16-allele site: not linkable
static const uint32_t kSites = sizeof(kAlleles) / sizeof(kAlleles[0]);

static uint32_t a_of(uint64_t s) { return s < kSites ? gmx_link_alleles(kAlleles[s]) : 0u; }

static int check(uint32_t span, const std::vector<std::pair<uint32_t, uint32_t>> &loci, bool lead, const char *what) {
  std::vector<uint64_t> off(kSites + 1);
  gmx_link_offsets(kSites, span, [](uint64_t s) { return kAlleles[s]; }, off.data());
  std::vector<GmxLinkSite> table(kSites);
  for (uint32_t s = 0; s < kSites; ++s) {
    uint32_t f = 0;
    for (uint32_t k = 0; k < 8; ++k) f |= a_of(s + k) << (4 * k);
    table[s] = GmxLinkSite{(uint32_t)off[s], f};
  }
  std::vector<uint32_t> got(off[kSites] + 1, 0), want(off[kSites] + 1, 0);  // (+ 1: a guard word no pair may touch)
  for (size_t i = 0; i < loci.size(); ++i)
    for (size_t j = i + 1; j < loci.size(); ++j) {
      const uint32_t si = loci[i].first, sj = loci[j].first, d = sj - si;
      if (d < 1 || d > span || loci[i].second >= a_of(si) || loci[j].second >= a_of(sj)) continue;
      uint64_t at = off[si];
      for (uint32_t e = 1; e < d; ++e) at += (uint64_t)a_of(si) * a_of(si + e);
      want[at + (uint64_t)loci[i].second * a_of(sj) + loci[j].second] += 1;
    }
  // the path: with `lead` the first locus is the allele the read starts inside (an inline handle; its allele is the first node's)
  ListEnv env;
  const size_t first = lead ? 1 : 0;
  for (size_t i = first; i < loci.size(); ++i)
    env.arena.push_back(GmxPathNode{5u + 2u * loci[i].first, (int32_t)loci[i].second, i + 1 < loci.size() ? (uint32_t)(i + 1 - first) : GMX_NIL});
  GmxNode node{};
  node.site = lead ? 5u + 2u * loci[0].first : 0u;
  node.allele = lead ? (int32_t)loci[0].second : -1;
  const uint32_t pos_node[1] = {0u};
  GmxIndexView ix{};
  ix.nodes = &node;
  ix.pos_node = pos_node;
  GmxLinks lk{table.data(), got.data(), span, kSites};
  gmx_link_path(lk, ix, env, 0u, loci.size() > first ? 0u : GMX_NIL, lead ? (GMX_INLINE_FLAG | loci[0].first) : GMX_NIL);
  if (got != want) {
    std::printf("FAILED %s span %u\n", what, span);
    for (size_t w = 0; w < got.size(); ++w)
      if (got[w] != want[w]) std::printf("  word %zu: got %u want %u\n", w, got[w], want[w]);
    return 1;
  }
  return 0;
}

int main() {
  int bad = 0, n = 0;
  for (uint32_t span = 1; span <= GMX_LINK_MAX_SPAN; ++span) {
    // all fifteen sites: three batch boundaries, both non-linkable sites in the middle, pairs seven apart
    std::vector<std::pair<uint32_t, uint32_t>> all;
    for (uint32_t s = 0; s < kSites; ++s) all.push_back({s, (s * 7u + 1u) % (kAlleles[s] < 8 ? kAlleles[s] : 8u)});
    bad += check(span, all, false, "every site"), ++n;
    bad += check(span, all, true, "every site, starting inside the first"), ++n;
    // exactly four and five loci: the batch's edge; an allele of 15, of 200 and one out of range by one add nothing
    bad += check(span, {{0, 1}, {1, 2}, {2, 3}, {3, 0}}, false, "four loci"), ++n;
    bad += check(span, {{5, 2}, {6, 1}, {7, 15}, {8, 7}, {9, 200}}, false, "alleles beyond range"), ++n;
    bad += check(span, {{1, 3}, {2, 0}, {3, 1}}, true, "the leading allele out of range by one"), ++n;
    // sites that are not neighbours, the last site, one locus, none
    bad += check(span, {{0, 0}, {3, 1}, {7, 3}, {14, 1}}, false, "gaps"), ++n;
    bad += check(span, {{12, 1}, {14, 0}}, true, "across the 16-allele site"), ++n;
    bad += check(span, {{6, 1}}, false, "one locus"), ++n;
    bad += check(span, {{6, 1}}, true, "only the allele it starts inside"), ++n;
    bad += check(span, {}, false, "no locus"), ++n;
  }
  if (bad) return 1;
  std::printf("ok %d\n", n);
  return 0;
}

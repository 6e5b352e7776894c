"""Shared by test_strand_bias_host.py (no GPU) and test_strand_log.py (GPU): the definitions of COV_FWD, COV_REV and SB
(include/gmx.h, gmx_infer_annotate_strands) restated in Python, the exact Fisher probability, and the removal of the three
fields from the call files."""
import math
import re

from gramtools_amd.quasimap import LOG_COUNTED


def counted(site, ids, count):
    """A counted grouped-log record."""
    return [site, len(ids) | LOG_COUNTED, count & 0xFFFFFFFF, count >> 32, *ids]


def exact_phred(a, b, c, d):
    """-10 log10 of the two-sided Fisher exact probability of [[a, b], [c, d]] in integer arithmetic: the tables with the same
    margins weigh C(r1, x) C(r2, c1 - x) out of C(n, c1); those of at most the observed weight times (1 + 1e-7) are summed."""
    r1, r2, c1 = a + b, c + d, a + c
    if 0 in (r1, r2, c1, b + d):
        return 0.0
    lo, hi = max(0, c1 - r2), min(r1, c1)
    w = math.comb(r1, lo) * math.comb(r2, c1 - lo)
    weights = [w]
    for x in range(lo, hi):  # w(x + 1) from w(x): exact
        w = w * (r1 - x) * (c1 - x) // ((x + 1) * (r2 - c1 + x + 1))
        weights.append(w)
    total = sum(weights)
    assert total == math.comb(r1 + r2, c1)
    obs = weights[a - lo]
    num = sum(v for v in weights if v * 10 ** 7 <= obs * (10 ** 7 + 1))
    if num >= total:
        return 0.0
    return -10.0 * (math.log10(num) - math.log10(total))  # (math.log10 of an int is exact to a double's precision at any size)


def haploid(groups, h):
    return sum(c for ids, c in groups.items() if h in ids)


def expected_fields(site, groups_fwd, groups_rev, hapg_of_allele):
    """The three fields of a site that has a call, from its jVCF object and the site's grouped counts per strand
    ({ids: count}); hapg_of_allele: the haplogroup of every output allele (None: not known to the test)."""
    called = set(site["HAPG"][0])
    table = []
    for groups in (groups_fwd, groups_rev):
        hit = sum(c for ids, c in groups.items() if called & set(ids))
        table.append((hit, sum(groups.values()) - hit))
    (cf, of), (cr, orv) = table
    return dict(COV_FWD=[None if h is None else haploid(groups_fwd, h) for h in hapg_of_allele],
                COV_REV=[None if h is None else haploid(groups_rev, h) for h in hapg_of_allele],
                SB=exact_phred(cf, cr, of, orv))


def strip_json(text):
    """genotyped.json without the three fields and their descriptions."""
    text = re.sub(r'"COV_FWD":\{"Desc":"[^"]*"\},"COV_REV":\{"Desc":"[^"]*"\},', "", text)
    text = re.sub(r'"SB":\{"Desc":"[^"]*"\},', "", text)
    text = re.sub(r',"COV_FWD":\[\[[0-9,]*\]\],"COV_REV":\[\[[0-9,]*\]\]', "", text)
    return re.sub(r',"SB":\[[^\]]*\]', "", text)


def strip_vcf(text):
    """The VCF text without the three FORMAT entries, their header lines and their values."""
    out = []
    for line in text.splitlines(keepends=True):
        if re.match(r"##FORMAT=<ID=(COV_FWD|COV_REV|SB),", line):
            continue
        if not line.startswith("#"):
            f = line.rstrip("\n").split("\t")
            assert f[8].endswith(":COV_FWD:COV_REV:SB"), line
            f[8] = f[8][:-len(":COV_FWD:COV_REV:SB")]
            f[9] = ":".join(f[9].split(":")[:-3])
            line = "\t".join(f) + "\n"
        out.append(line)
    return "".join(out)

"""Inputs of tests/test_gpu_cli_paths.py, built without a GPU so that tests/test_cli_paths_inputs.py can check on the CPU that they
hold what the GPU test is about: a three-contig FASTA of 3 000 planted bases each, two callsets, a -b BED and a --stratify list.

chrA has a dozen phased records in both callsets, chrB has records in the truth VCF only, chrC is named by the BED and by both VCF
headers and has no record: it is evaluated with zero superclusters."""
import numpy as np

import context_cases as CC
import longrepeats_cases as LC

NAMES = ["chrA", "chrB", "chrC"]
LENGTH = 3000
WORD_SITES = (500, 600, 700, 800, 900, 1000)           # chrA: the six low-complexity words of context_cases.PLANTS
GC_SITES = (700, 1100, 1500, 1900, 2300)               # chrB: 400 bases of fixed GC content around each

# chrA, 0-based: (position, kind, truth GT, query GT or None, phase set).  Kinds: snp, ins (two bases), del (two bases).
CHR_A = [(150, "snp", "0|1", "0|1", 151), (500, "snp", "1|0", "1|0", 151), (800, "snp", "0|1", "0|1", 151),
         (1200, "snp", "0|1", "0|1", 151), (1210, "snp", "1|0", "1|0", 151), (1300, "snp", "0|1", None, 151),      # (a truth FN)
         (1400, "ins", "0|1", "0|1", 151), (1600, "del", "1|0", "1|0", 1601), (1700, "snp", "0|1", "1|0", 1601),   # (a flipped phase)
         (1900, "snp", "1|1", "0|1", 1601),                                                                        # (hom against het)
         (2100, "snp", "0|1", "0|1", 1601), (2200, "snp", None, "0|1", 1601),                                      # (a query FP)
         (2700, "snp", "1|0", "1|0", 1601)]
CHR_B = [(150, "snp", "0|1", None, 151), (900, "snp", "1|1", None, 151), (2700, "snp", "1|0", None, 151)]
BED = [("chrA", 50, 2950), ("chrB", 50, 2950), ("chrC", 0, 3000)]
STRATA = [("left", [("chrA", 0, 1500), ("chrB", 0, 1500)]), ("right", [("chrA", 1500, 3000), ("chrC", 0, 3000)])]


def contigs():
    """the three contigs: a forward copy of 300 bases on chrA and chrB and a reverse-complemented one on chrC and chrA (every
    default repeat and long repeat stratum has intervals on all three), the context words on chrA and the GC bands on chrB"""
    g = LC.Genome(77, (LENGTH,) * 3)
    g.forward(250, 0, 100, 1, 100, g.r(300))
    g.reverse(250, 2, 100, 0, 2600, g.r(300))
    seqs = [np.frombuffer(bytes(s), np.uint8).copy() for s in g.ctg]
    rng = np.random.RandomState(78)
    CC.plant_defaults(seqs[0], WORD_SITES, rng)
    for pc, p in zip(CC.GC_PERCENT, GC_SITES):
        seqs[1][p - 200:p + 200] = CC.periodic_gc(rng, pc)
    return [bytes(s) for s in seqs]


def hap_variants(records, query):
    """hap-variants a callset's records give: one for a heterozygous record, two for a homozygous one"""
    return sum(gt.count("1") for gt in (r[3 if query else 2] for r in records) if gt)


def vcf(ctgs, query):
    """the text of the truth (query false) or the query VCF; the header names all three contigs"""
    out = ["##fileformat=VCFv4.2"] + [f"##contig=<ID={n},length={len(c)}>" for n, c in zip(NAMES, ctgs)]
    out += ['##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">', '##FORMAT=<ID=PS,Number=1,Type=Integer,Description="Phase set">',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    for name, seq, records in ((NAMES[0], ctgs[0], CHR_A), (NAMES[1], ctgs[1], CHR_B)):
        for pos, kind, t_gt, q_gt, ps in records:
            gt = q_gt if query else t_gt
            if gt is None:
                continue
            base = chr(seq[pos])
            other = "ACGT"["ACGT".index(base) - 3]
            ref, alt = {"snp": (base, other), "ins": (base, base + "GT"), "del": (seq[pos:pos + 3].decode(), base)}[kind]
            out.append(f"{name}\t{pos + 1}\t.\t{ref}\t{alt}\t30\tPASS\t.\tGT:PS\t{gt}:{ps}")
    return "\n".join(out) + "\n"


def write(tmp):
    """the files under tmp -> dict(inputs=[query, truth, fasta, "-b", bed], list=the --stratify list, contigs=the sequences)"""
    import strata_model as SM
    ctgs = contigs()
    (tmp / "three.fa").write_text("".join(f">{n}\n{c.decode()}\n" for n, c in zip(NAMES, ctgs)))
    (tmp / "truth.vcf").write_text(vcf(ctgs, False))
    (tmp / "query.vcf").write_text(vcf(ctgs, True))
    (tmp / "regions.bed").write_text("".join(f"{c}\t{a}\t{b}\n" for c, a, b in BED))
    lst = SM.write_strata(tmp, STRATA, "strata.tsv")
    return dict(inputs=[str(tmp / "query.vcf"), str(tmp / "truth.vcf"), str(tmp / "three.fa"), "-b", str(tmp / "regions.bed")], list=lst,
                contigs=ctgs)

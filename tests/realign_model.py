"""CPU model of the realignment (-rq / -rt, include/vcfdist_realign.h), restated plainly from the reference (vcfdist v2.6.4):
wf_swg_realign (dist.cpp:2496-2594) with generate_str (dist.cpp:81-138), add_variants (variant.cpp:332-391), left_shift
(variant.cpp:57-127) and write_vcf / print_variant (variant.cpp:132-222, 292-315).  The alignment itself is the CPU
wf_swg_align + wf_swg_backtrack of tests/distance_model.cpp (distance_helpers.steps: forward steps of the reversed strings).

A hap is a dict of the reader's columns (vcfdist_amd.io): pos, rlen, type, ref_len, alt_len, ref_off, alt_off, pool, var_qual,
phase_set and optionally gt_qual, orig_gt."""
import datetime

import numpy as np

import distance_helpers as DH

SUB, INS, DEL = 1, 2, 3
F_INS, F_DEL, F_MAT, F_SUB = 1, 2, 4, 8
ST_EDGE, ST_LIMIT, ST_ERROR = 1, 2, 4
GT_REF_REF = 2
COLS = ("pos", "rlen", "type", "ref_len", "alt_len", "var_qual", "gt_qual", "phase_set", "orig_gt")


def alleles(hap, i):
    p = hap["pool"]
    r0, a0 = int(hap["ref_off"][i]), int(hap["alt_off"][i])
    return bytes(p[r0:r0 + int(hap["ref_len"][i])]).decode(), bytes(p[a0:a0 + int(hap["alt_len"][i])]).decode()


def generate_str(seq, hap, b, e, beg, end):
    """generate_str over [beg, end) with the cluster's variants b..e-1; None where the reference ERRORs or throws (the walk goes
    backwards, or a reference piece starts past the contig's end)"""
    out, v, pos = [], b, beg
    while pos < end:
        if v < e and pos == hap["pos"][v]:
            t = hap["type"][v]
            ref, alt = alleles(hap, v)
            if t == INS:
                out.append(alt)
            elif t == DEL:
                pos += len(ref)
            else:
                out.append(alt)
                pos += 1
            v += 1
        else:
            stop = min(end, int(hap["pos"][v])) if v < e else end
            if stop < pos or pos > len(seq):
                return None
            out.append(seq[pos:stop])
            pos = stop
    return "".join(out)


def add_variants(steps, beg, query, ref):
    """the CIGAR (forward steps) into (pos, type, ref, alt) records: one SUB per base, DEL runs, INS runs"""
    recs, qi, ri, k = [], 0, 0, 0
    while k < len(steps):
        s = steps[k]
        if s == F_MAT:
            qi += 1; ri += 1; k += 1
        elif s == F_SUB:
            recs.append((beg + ri, SUB, ref[ri], query[qi]))
            qi += 1; ri += 1; k += 1
        else:
            n = 0
            while k < len(steps) and steps[k] == s:
                n += 1; k += 1
            if s == F_DEL:
                recs.append((beg + ri, DEL, ref[ri:ri + n], ""))
                ri += n
            else:
                recs.append((beg + ri, INS, "", query[qi:qi + n]))
                qi += n
    return recs


def realign_cluster(seq, hap, b, e, x=5, o=6, ex=2):
    """-> (status, records): status ST_EDGE / ST_ERROR where the cluster keeps its variants"""
    beg = int(hap["pos"][b]) - 1
    end = int(hap["pos"][e - 1]) + int(hap["rlen"][e - 1]) + 1
    if beg < 0:
        return ST_EDGE, None
    if beg > len(seq):
        return ST_ERROR, None
    query = generate_str(seq, hap, b, e, beg, end)
    ref = seq[beg:end]
    if query is None or not query or not ref:
        return ST_ERROR, None
    return 0, add_variants(DH.steps(query, ref, x, o, ex), beg, query, ref)


def realign(seq, hap, var_beg, x=5, o=6, e=2, max_qual=60, keep=None):
    """wf_swg_realign + left_shift of one (contig, hap).  var_beg: the clusters (n + 1 entries); keep: per-cluster status bits
    decided elsewhere (the device's VRL_ST_LIMIT), such clusters keep their variants.  -> (list of record dicts, status array)"""
    seq = seq if isinstance(seq, str) else bytes(np.asarray(seq, np.uint8)).decode()
    n_cl = max(len(var_beg) - 1, 0) if len(hap["pos"]) else 0
    status = np.zeros(n_cl, np.uint8)
    out = []
    for c in range(n_cl):
        b, en = int(var_beg[c]), int(var_beg[c + 1])
        st, recs = (int(keep[c]), None) if keep is not None and keep[c] else realign_cluster(seq, hap, b, en, x, o, e)
        status[c] = st
        if st:
            for v in range(b, en):
                ref, alt = alleles(hap, v)
                out.append(dict(pos=int(hap["pos"][v]), rlen=int(hap["rlen"][v]), type=int(hap["type"][v]), ref=ref, alt=alt,
                                var_qual=np.float32(hap["var_qual"][v]),
                                gt_qual=np.float32(hap["gt_qual"][v]) if "gt_qual" in hap else np.float32(max_qual),
                                phase_set=int(hap["phase_set"][v]), orig_gt=int(hap["orig_gt"][v]) if "orig_gt" in hap else GT_REF_REF))
            continue
        qual = np.float32(max_qual)
        for v in range(b, en):
            qual = min(qual, np.float32(hap["var_qual"][v]))
        ps = next((int(p) for p in hap["phase_set"][b:en] if p != 0), 0)
        for pos, t, ref, alt in recs:
            out.append(dict(pos=pos, rlen=len(ref), type=t, ref=ref, alt=alt, var_qual=np.float32(int(qual)), gt_qual=np.float32(max_qual),
                            phase_set=ps, orig_gt=GT_REF_REF))
    left_shift(out, seq)
    return out, status


def left_shift(recs, seq):
    for i, r in enumerate(recs):
        if r["type"] not in (INS, DEL):
            continue
        key = "alt" if r["type"] == INS else "ref"
        while r["pos"] > 0 and r["pos"] - 1 < len(seq) and (i == 0 or r["pos"] > recs[i - 1]["pos"] + recs[i - 1]["rlen"] + 1):
            base = seq[r["pos"] - 1]
            if base != r[key][-1]:
                break
            r[key] = base + r[key][:-1]
            r["pos"] -= 1
    for i in range(len(recs) - 1):
        a, b = recs[i], recs[i + 1]
        if a["ref"] and b["pos"] == a["pos"]:
            for k in ("rlen", "type", "ref", "alt", "orig_gt", "gt_qual", "var_qual"):
                a[k], b[k] = b[k], a[k]


def columns(recs):
    """records -> the reader's column dict (pool: REF then ALT of each record in order)"""
    n = len(recs)
    d = {k: np.zeros(n, dt) for k, dt in (("pos", np.int32), ("rlen", np.int32), ("type", np.uint8), ("ref_len", np.int32),
                                         ("alt_len", np.int32), ("ref_off", np.int64), ("alt_off", np.int64), ("var_qual", np.float32),
                                         ("gt_qual", np.float32), ("phase_set", np.int32), ("orig_gt", np.uint8))}
    pool = bytearray()
    for i, r in enumerate(recs):
        for k in ("pos", "rlen", "type", "var_qual", "gt_qual", "phase_set", "orig_gt"):
            d[k][i] = r[k]
        d["ref_len"][i], d["alt_len"][i] = len(r["ref"]), len(r["alt"])
        d["ref_off"][i] = len(pool); pool += r["ref"].encode()
        d["alt_off"][i] = len(pool); pool += r["alt"].encode()
    d["pool"] = np.frombuffer(bytes(pool) + b"\0", np.uint8).copy()
    return d


def records(hap):
    """the reader's column dict -> records (for comparisons: allele strings instead of pool offsets)"""
    out = []
    for i in range(len(hap["pos"])):
        ref, alt = alleles(hap, i)
        out.append(dict(pos=int(hap["pos"][i]), rlen=int(hap["rlen"][i]), type=int(hap["type"][i]), ref=ref, alt=alt,
                        var_qual=np.float32(hap["var_qual"][i]), gt_qual=np.float32(hap["gt_qual"][i]), phase_set=int(hap["phase_set"][i]),
                        orig_gt=int(hap["orig_gt"][i])))
    return out


def write_vcf(contigs, sample, fasta, file_date=None):
    """variantData::write_vcf -> text.  contigs: [(name, length, ploidy, [records hap 1, records hap 2])]"""
    if file_date is None:
        file_date = datetime.date.today().strftime("%Y%m%d")
    lines = ["##fileformat=VCFv4.2", "##fileDate=" + file_date]
    lines += ["##contig=<ID=%s,length=%d,ploidy=%d>" % (n, ln, p) for n, ln, p, _ in contigs]
    lines += ['##FILTER=<ID=PASS,Description="All filters passed">', '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    for name, _, ploidy, haps in contigs:
        seq = fasta.get(name) if fasta else None

        def line(r, pos, gt):
            ref, alt = r["ref"], r["alt"]
            if r["type"] in (INS, DEL):
                base = chr(seq[pos]) if not isinstance(seq, str) else seq[pos]
                ref, alt = base + ref, base + alt
            return "%s\t%d\t.\t%s\t%s\t%f\tPASS\t.\tGT\t%s" % (name, pos + 1, ref, alt, float(r["var_qual"]), gt)
        p = [0, 0]
        while p[0] < len(haps[0]) or p[1] < len(haps[1]):
            at = [haps[h][p[h]]["pos"] - (haps[h][p[h]]["type"] in (INS, DEL)) if p[h] < len(haps[h]) else 2 ** 31 - 1 for h in (0, 1)]
            pos = min(at)
            h1, h2 = at[0] == pos, at[1] == pos
            if h1 and h2:
                a, b = haps[0][p[0]], haps[1][p[1]]
                if a["ref"] == b["ref"] and a["alt"] == b["alt"]:
                    lines.append(line(a, pos, "1|1"))
                else:
                    lines += [line(a, pos, "1|0"), line(b, pos, "0|1")]
            elif h1:
                lines.append(line(haps[0][p[0]], pos, "1" if ploidy == 1 else "1|0"))
            else:
                lines.append(line(haps[1][p[1]], pos, "1" if ploidy == 1 else "0|1"))
            p[0] += h1
            p[1] += h2
    return "\n".join(lines) + "\n"

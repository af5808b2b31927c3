"""What tests/test_decode_annot_model.py (host, no GPU), tests/test_gpu_decode_annot.py and
tests/test_cli_decode_annotate_gpu.py share: the expected text of `decode --annotate`, built from the decoder's output
WITHOUT the option and tests/annot_model.py, never from the code under test; BED files written against a database's @SQ
lines; and the small synthetic databases of the GPU tests.

The rule (gs_annot_scan.h, gs_an_decoded_footprint): an off-target printed at position x on strand '+' of a record whose
stored SEQ has n symbols occupies [x + 1 - n, x + 1), on '-' [x, x + n), clipped to [0, LN).  annot_model.row_features
takes a row printed at s with width w and looks at [s - 1, s - 1 + w) clipped to [0, length): s = x + 2 - n for '+',
s = x + 1 for '-', w = n, length = LN say the same interval in its terms."""
import annot_model as am
import decode_golden as dg

decode = dg.decode

COMPLETE_COLUMN = b",match_features"
SUCCINCT_COLUMNS = b"".join(b",distance_%d_feature_matches" % k for k in range(4))


def generic_bed(sq, skip=()):
    """intervals on every chromosome of sq but those in `skip`: the first and the last base, a gene over the middle half
    with exons of two alternating groups inside it, three groups stacked over one base, two abutting intervals"""
    rows = []
    for name, ln in sq:
        if name in skip or ln < 8:
            continue
        rows += [f"{name}\t0\t1\tfirst_base", f"{name}\t{ln - 1}\t{ln}\tlast_base", f"{name}\t{ln // 4}\t{3 * ln // 4}\tgene_{name}"]
        step = max(7, ln // 40)
        for i, at in enumerate(range(ln // 4, 3 * ln // 4 - 3, step)):
            rows.append(f"{name} {at} {at + 3} exon_{'odd' if i & 1 else 'even'}")
        mid = ln // 2
        rows += [f"{name}\t{mid}\t{mid + 1}\tstack_{k}" for k in range(3)]
        rows += [f"{name}\t{ln // 8}\t{ln // 8 + 2}", f"{name}\t{ln // 8 + 2}\t{ln // 8 + 4}\tabuts"]
    return "# written against the @SQ lines\n" + "\n".join(rows) + "\n"


def row_column(fields, n, lengths, lines, names):
    """the features of a complete-mode row from the fields it prints (…, chromosome, position, sense, …) and the stored
    length n of its record's SEQ -> (group numbers, the column's text)"""
    chrom, x, sense = fields[3], int(fields[4]), fields[5]
    s = x + 2 - n if sense == "+" else x + 1
    feats = am.row_features(chrom, s, n, lengths[chrom], lines)
    return feats, am.column(feats, names)


def split_complete(row):
    """id,match_number,sequence,chromosome,position,sense,distance,cfd - the id may hold commas, the rest does not"""
    f = row.rsplit(",", 7)
    assert len(f) == 8, row
    return f


def seq_lengths(records):
    """id -> the stored SEQ's length; the rows name their record by its id, so the ids must tell the records apart"""
    out = {}
    for r in records:
        assert out.setdefault(r.id, len(r.seq)) == len(r.seq), f"two records named {r.id} with SEQ of different lengths"
    return out


def expected_complete(plain, sq, records, bed, header=True, features_only=False):
    """plain: the complete-mode table without the option (bytes) -> (the table with it, the features row by row)"""
    names, lines = am.bed_lines(bed)
    lengths, n_of = dict(sq), seq_lengths(records)
    assert len(lengths) == len(sq)
    rows = plain.decode("latin-1").split("\n")
    assert rows[-1] == ""
    out, seen = [], []
    if header:
        out.append(rows[0] + COMPLETE_COLUMN.decode())
    for row in rows[1 if header else 0:-1]:
        f = split_complete(row)
        feats, col = row_column(f, n_of[f[0]], lengths, lines, names)
        seen.append(feats)
        if features_only and not feats:
            continue
        out.append(row + "," + col)
    return ("\n".join(out) + "\n" if out else "").encode("latin-1"), seen


def expected_succinct(plain, plain_complete, sq, records, bed, header=True):
    """plain: the succinct table without the option; plain_complete: the complete one of the same records, with its
    header line (the off-targets are counted from its rows: every row of the record at that distance that has a feature)"""
    names, lines = am.bed_lines(bed)
    lengths = dict(sq)
    # the complete table's rows in groups, one per record that has off-targets: match_number counts from 0 in each
    groups = []
    for row in plain_complete.decode("latin-1").split("\n")[1:-1]:
        f = split_complete(row)
        if f[1] == "0":
            groups.append([])
        groups[-1].append(f)
    rows = plain.decode("latin-1").split("\n")
    out = [rows[0] + SUCCINCT_COLUMNS.decode()] if header else []
    body = rows[1 if header else 0:-1]
    assert len(body) == len(records)
    at = 0
    for row, rec in zip(body, records):
        assert row.startswith(rec.id + ",")
        printed = [int(v) for v in row.rsplit(",", 5)[1:5]]     # distance_0_matches .. distance_3_matches
        counts = [0, 0, 0, 0]
        if sum(printed):
            group = groups[at]
            at += 1
            assert group[0][0] == rec.id and len(group) == sum(printed)
            for f in group:
                if row_column(f, len(rec.seq), lengths, lines, names)[0]:
                    counts[int(f[6])] += 1
        out.append(row + "".join(f",{v}" for v in counts))
    assert at == len(groups)
    return ("\n".join(out) + "\n" if out else "").encode("latin-1")


# ---- the synthetic database of the GPU tests ------------------------------------------------------------------------
SQ = [("cA", 97), ("cB", 64), ("cC", 40), ("cD", 50)]
N = 23


def small_genome():
    """four chromosomes of 97, 64, 40 and 50 bases over A,C,G,T (no N: a 23-symbol slice never fails on its PAM).  cC's
    FASTA record is shorter than its LN: the printed slice is cut there, the footprint is not"""
    import numpy as np
    rng = np.random.default_rng(5)
    fasta = {name: "".join(rng.choice(list("ACGT"), ln)) for name, ln in SQ}
    fasta["cC"] = fasta["cC"][:31]
    return fasta


def small_bed():
    """cA: the first base, the last base, abutting intervals with a repeated group under a gene with an exon (a '+'
    footprint that ends at 52 is [30, 53): six elementary segments, `rep` over the first and the fifth of them: the merge).
    cB: one base under two groups.  cC: absent.  cD: intervals but no off-target in the database."""
    rows = ["cA\t0\t1\tfirst_base", "cA\t96\t97\tlast_base",
            "cA\t28\t34\trep", "cA\t34\t40\tmid", "cA\t40\t46\trep", "cA\t46\t60\ttail", "cA\t30\t58\tgene", "cA 36 38 exon",
            "cA\t21\t22\tbase_21",
            "cB\t63\t64\tlast_base", "cB\t0\t2\thead", "cB\t20\t21\tdot_a", "cB\t20\t21\tdot_b",
            "cD\t5\t45\tnever_hit"]
    return "\n".join(rows) + "\n"


def word(chrom, x, strand):
    """the database word of the off-target at x on `chrom`"""
    cum = 0
    for name, ln in SQ:
        if name == chrom:
            assert 0 <= x < ln
            v = cum + x
            assert v != 0 or strand == "-", "the word 0 reads as '-' (the script tests word > 0)"
            return v if strand == "+" else -v
        cum += ln
    raise KeyError(chrom)


def delim():
    return -(sum(ln for _, ln in SQ) + 1)


def hex_list(groups):
    """[(distance, [words])] -> the of:H: digits"""
    lst = []
    for d, words in groups:
        lst += list(words) + [d, delim()]
    return dg.hexw(lst)


def small_records():
    """The records of the synthetic database, every stored SEQ of 23 symbols unless said otherwise:
       edges     off-targets at x = 0, n - 2, n - 1 and LN - 1 of cA, cB and cC on both strands: both clips, and footprints
                 of one base
       merge     a footprint over four elementary segments with a repeated group
       big66/big130/big200  more than 64 off-target words each (k_dc_fold loads 64 at a time; complete-mode tiles straddle
                 the records' boundaries: the lists are 66 + 8, 130 + 8 and 200 + 8 words long)
       no_of     no of field;  unmapped  RNAME '*';  short20  a stored SEQ of 20 symbols;  rev  FLAG 16
       desert    130 off-targets on cC, which the BED file does not name: wherever the list begins, one tile of 64 slots
                 lies inside it and has, under features-only, no row at all
    cD has intervals and no off-target.  -> [decode.Record]"""
    import numpy as np
    rng = np.random.default_rng(9)
    fasta = small_genome()
    guide = "ACGTTGCAAGCTTGCATGCAAGG"

    def rec(name, groups, seq=guide, rev=False, rname="cA", pos0=3):
        return decode.Record(name, seq, rev, rname, pos0, hex_list(groups) if groups is not None else None)

    edges = []
    for chrom, ln in SQ[:3]:
        for x in (0, N - 2, N - 1, ln - 1):
            for strand in "+-":
                if chrom == "cA" and x == 0 and strand == "+":
                    continue
                edges.append(word(chrom, x, strand))
    recs = [rec("edges", [(0, edges[:5]), (1, edges[5:11]), (2, []), (3, edges[11:])])]
    recs.append(rec("merge", [(0, [word("cA", 52, "+"), word("cA", 30, "-")]), (1, [word("cA", 36, "+")])]))
    for n in (66, 130, 200):
        ws = [word("cA", int(x), "+-"[int(s)]) for x, s in zip(rng.integers(1, 97, n), rng.integers(0, 2, n))]
        ws += [word("cB", int(x), "+") for x in rng.integers(0, 64, 4)]
        cut = sorted(int(c) for c in rng.integers(0, len(ws) + 1, 3))
        recs.append(rec(f"big{n}", [(0, ws[:cut[0]]), (1, ws[cut[0]:cut[1]]), (2, ws[cut[1]:cut[2]]), (3, ws[cut[2]:])],
                        rev=n == 130, rname="cB", pos0=n % 40))
    recs.append(rec("no_of", None))
    recs.append(rec("unmapped", [(1, [word("cB", 20, "+"), word("cB", 20, "-")])], rname=None, pos0=-1))
    recs.append(rec("short20", [(0, [word("cA", 19, "+"), word("cA", 96, "-"), word("cB", 62, "-")])], seq=guide[:20]))
    recs.append(rec("rev", [(2, [word("cA", 33, "-"), word("cC", 39, "+"), word("cC", 35, "-")])], rev=True, rname="cC", pos0=10))
    recs.append(rec("desert", [(3, [word("cC", int(x), "+-"[i & 1]) for i, x in enumerate(rng.integers(0, 40, 130))])]))
    recs.append(rec("after", [(0, [word("cA", 0, "-"), word("cB", 63, "-")])]))
    assert all(len(r.seq) <= 32 for r in recs) and fasta
    return recs


def sam_text(records, sq=SQ):
    import bam_make as bm
    head = "@HD\tVN:1.0\tSO:unknown\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in sq)
    return head + "".join(bm.sam_line(r.id, 16 if r.reverse else 0, r.rname, r.pos0, r.seq, [r.hex] if r.hex is not None else [])
                          for r in records)


def write_fasta(path, fasta):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in fasta.items()))

#!/usr/bin/env python3
"""Writes tests/golden/decode/: SAM databases, their FASTA files and what the REFERENCE's own
scripts/decode_database.py prints for them in both modes.  Build-container only (needs /root/reference).

The script cannot be imported here: pysam and Biopython are missing.  As in tools/make_kmers_goldens.py its top-level
assignments and function definitions are compiled with `ast` where the file lies (`__file__` set, so that its score
pickles load) and driven as its __main__ block drives them, with two stand-ins: an object with the attributes the
script reads of a pysam record, and a `str` subclass for the Bio.Seq of a FASTA record.  Nothing of the script or of
the pickles' code is kept in this repository: the fixtures hold inputs, expected text, the exception's name where
the script raises, and the 240 + 16 score values as numbers (cfd_tables.json).

The left fold of sum() over floats is the contract (compensated from Python 3.12 on): refuses to run there.
"""
import ast
import binascii
import contextlib
import io
import json
import os
import pickle
import struct
import sys
from functools import reduce
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference/scripts/decode_database.py")
OUT = ROOT / "tests" / "golden" / "decode"
TOY = ROOT / "tests" / "golden" / "toy"


def reference_functions():
    tree = ast.parse(REF.read_text(), filename=str(REF))
    keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.Assign))]
    ns = dict(__file__=str(REF), os=os, pickle=pickle, np=np, binascii=binascii, reduce=reduce, sys=sys)
    exec(compile(ast.Module(body=keep, type_ignores=[]), str(REF), "exec"), ns)
    return ns


class Seq(str):
    def __getitem__(self, k):
        return Seq(str.__getitem__(self, k))

    def upper(self):
        return Seq(str.upper(self))


class FastaRecord:
    def __init__(self, seq):
        self.seq = Seq(seq)


class SamRecord:
    def __init__(self, line, names):
        f = line.split("\t")
        self.query_name, self.flag, self.query_sequence = f[0], int(f[1]), f[9]
        # htslib treats an RNAME that no @SQ line names as it treats '*': unmapped, and pysam gives None for it
        self.reference_name = f[2] if f[2] in names else None
        self.reference_start = int(f[3]) - 1
        self.is_reverse = bool(self.flag & 16)
        self.tags = {t[:2]: t[5:] for t in f[11:]}

    def has_tag(self, t):
        return t in self.tags

    def get_tag(self, t):
        return self.tags[t]


def read_fasta(path):
    recs, name = {}, None
    for line in Path(path).read_text().splitlines():
        if line.startswith(">"):
            name = line[1:].split()[0]
            recs[name] = []
        else:
            recs[name].append(line.strip())
    return {k: FastaRecord("".join(v)) for k, v in recs.items()}


def run_script(ns, sam_text, fasta, mode):
    """what the script's __main__ prints, or {"raises": name}"""
    lines = sam_text.splitlines()
    genome = []
    for ln in lines:
        if ln.startswith("@SQ"):
            t = dict(x.split(":", 1) for x in ln.split("\t")[1:])
            genome.append({"SN": t["SN"], "LN": int(t["LN"])})
    delim = ns["get_nonexist_int_coord"](genome)
    names = {g["SN"] for g in genome}
    records = [SamRecord(ln, names) for ln in lines if ln and not ln.startswith("@")]
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            if mode == "succinct":
                print(ns["SUCCINCT_HEADER"])
                for r in records:
                    ns["output_succinct"](r, list(ns["decode_off_targets"](r, genome, delim, fasta)))
            else:
                print(ns["COMPLETE_HEADER"])
                for r in records:
                    ns["output_complete"](ns["decode_off_targets"](r, genome, delim, fasta))
    except Exception as e:  # the fixture records that the script fails, not what it had printed until then
        return {"raises": type(e).__name__}
    return buf.getvalue()


# ---- the hand-made set ------------------------------------------------------------------------------------------
def hexw(words):
    return "".join(struct.pack("<q", w).hex() for w in words)


def rc(s):
    return s[::-1].translate(str.maketrans("ACGTUN", "TGCAAN"))


def hand_made():
    rng = np.random.default_rng(11)
    ln = {"chrA": 1500, "chrB": 1200, "chrC": 900}
    seq = {k: list("".join(rng.choice(list("ACGT"), v))) for k, v in ln.items()}
    guide = "GACCTTGAGTCAGGATCCAT"
    site = guide + "AGG"

    def plant(ch, at, s):
        seq[ch][at:at + len(s)] = list(s)

    def mutate(s, where):
        s = list(s)
        for i in where:
            s[i] = "ACGT"[("ACGT".index(s[i]) + 1 + i % 3) % 4]
        return "".join(s)

    start = {"chrA": 0, "chrB": 1500, "chrC": 2700}
    total = 3600
    delim = -(total + 1)
    # perfect sites and neighbours on both strands
    plant("chrA", 100, site)
    plant("chrA", 300, mutate(site, [3]))
    plant("chrA", 400, rc(mutate(site, [5, 17])))
    plant("chrB", 200, mutate(site, [0, 9, 19]))
    plant("chrB", 500, rc(site))
    plant("chrC", 300, guide + "TGA")                       # PAM pair GA
    plant("chrC", 400, guide + "TTT")                       # PAM pair TT: score 0
    plant("chrC", 500, mutate(site, [1])[:6] + "N" + mutate(site, [1])[7:])   # N in the guide part: factor skipped
    plant("chrC", 600, guide[:4] + "R" + guide[5:] + "CGG")  # an IUPAC symbol
    plant("chrC", 700, guide[:9] + "U" + guide[10:] + "GGG")  # a U where the guide has T: equal after T->U
    plant("chrA", 800, guide + "ANG")                        # PAM pair NG: the script raises (kept out of the good sets)
    plant("chrA", 900, mutate(site, range(0, 20, 2))[:20] + "TGG")  # ten mismatches: exponent form
    plant("chrA", 1000, rc(mutate(site, range(1, 20, 2))[:20] + "CGG"))
    for p in range(1100, 1140):
        seq["chrA"][p] = "N"
    for p in range(1200, 1300):
        seq["chrA"][p] = seq["chrA"][p].lower()
    plant("chrA", 1250, site.lower())
    plant("chrA", 0, site)                                   # the first 23 bases of the genome
    plant("chrC", 900 - 23, rc(site))                        # the last 23 of the genome
    plant("chrB", 1100 - 23, site)                           # the end of chrB's FASTA record (shorter than its LN)
    text = {k: "".join(v) for k, v in seq.items()}
    text["chrB"] = text["chrB"][:1100]

    def plus(ch, at):   # the word of a '+' site that begins at `at`
        return start[ch] + at + 22

    def minus(ch, at):
        return -(start[ch] + at)

    sq = "".join(f"@SQ\tSN:{k}\tLN:{v}\n" for k, v in ln.items())
    head = "@HD\tVN:1.0\tSO:unknown\n" + sq

    def line(name, flag, ch, pos1, s, words, extra=""):
        of = "" if words is None else "\tof:H:" + hexw(words)
        return f"{name}\t{flag}\t{ch}\t{pos1}\t100\t{len(s)}M\t*\t0\t0\t{s}\t*\tk0:i:1{of}{extra}\tsp:f:0.500000\n"

    d0 = [plus("chrA", 100), minus("chrB", 500), plus("chrA", 0), minus("chrC", 877), plus("chrA", 1250)]
    d1 = [plus("chrA", 300), plus("chrC", 500), plus("chrC", 600)]
    d2 = [minus("chrA", 400)]
    d3 = [plus("chrB", 200)]
    good = []
    good.append(line("g_all", 0, "chrA", 101, site, d0 + [0, delim] + d1 + [1, delim] + d2 + [2, delim] + d3 + [3, delim]))
    good.append(line("g_rev", 16, "chrB", 501, rc(site), d0[:2] + [0, delim] + d1[:1] + [1, delim, 2, delim, 3, delim]))
    # PAM pairs: GA scores, TT is 0.0 (cfd empty; as the only off-target the sum is 0.0 and the specificity empty)
    good.append(line("g_pam_ga", 0, "chrC", 301, guide + "TGA", [plus("chrC", 300), plus("chrC", 700), 0, delim, 1, delim]))
    good.append(line("g_pam_zero", 0, "chrC", 401, guide + "TTT", [plus("chrC", 400), 0, delim]))
    good.append(line("g_pam_zero_mixed", 0, "chrC", 401, guide + "TTT", [plus("chrC", 400), plus("chrA", 100), 0, delim]))
    # many mismatches against 23-symbol slices: exponent form
    good.append(line("g_exp", 0, "chrA", 101, site, [plus("chrA", 100), 0, delim, plus("chrA", 900), minus("chrA", 1000), 3, delim]))
    # within n of every chromosome start and end, on both strands; word 0; the last base of the genome; the N run
    edge = []
    for ch in ("chrA", "chrB", "chrC"):
        for at in (0, 1, 5, 21, 22, 23):
            edge += [start[ch] + at, -(start[ch] + at)]
        for back in (1, 2, 5, 22, 23, 24):
            edge += [start[ch] + ln[ch] - back, -(start[ch] + ln[ch] - back)]
    edge = [w for w in edge if w != 0]
    edge += [start["chrB"] + 1100 - 1, -(start["chrB"] + 1100 - 23), -(start["chrB"] + 1100 - 10), start["chrB"] + 1150,
             -(start["chrB"] + 1150), start["chrA"] + 1145, -(start["chrA"] + 1095), total - 1, -(total - 1)]
    good.append(line("g_edges", 0, "chrA", 101, site, [plus("chrA", 100), 0, delim] + edge + [2, delim]))
    good.append(line("g_word0", 0, "chrA", 1, site, [0, plus("chrA", 0), 0, delim]))
    # 20 symbols without a PAM, 24 symbols, lower case as stored, no of field
    good.append(line("g_20", 0, "chrA", 101, guide, [start["chrA"] + 119, -(start["chrB"] + 503), 0, delim, start["chrA"] + 319, 1, delim]))
    good.append(line("g_24", 0, "chrA", 101, site + "A", [start["chrA"] + 123, 0, delim, start["chrC"] + 899, -(start["chrC"] + 877), 1, delim]))
    good.append(line("g_24_rev", 16, "chrA", 101, rc(site + "A"), [start["chrA"] + 123, 0, delim, total - 1, 1, delim]))
    good.append(line("g_lower", 0, "chrA", 1251, site.lower(), [plus("chrA", 1250), plus("chrA", 100), 0, delim]))
    good.append(line("g_no_of", 0, "chrA", 101, site, None))
    good.append(line("g_empty_of", 0, "chrA", 101, site, []))
    good.append(line("g_unmapped", 0, "*", 0, site, [plus("chrA", 100), 0, delim]))
    # empty groups, adjacent delims, words after the last delim, a lone delim, a lone distance
    good.append(line("g_groups", 0, "chrA", 101, site, [plus("chrA", 100), 0, delim, delim, 1, delim, delim, delim,
                                                        plus("chrB", 200), 3, delim, plus("chrA", 300), 1]))
    good.append(line("g_lone_delim", 0, "chrA", 101, site, [delim]))
    good.append(line("g_no_delim", 0, "chrA", 101, site, [plus("chrA", 100), 0]))
    good.append(line("g_upper_hex", 0, "chrA", 101, site, None, "\tof:H:" + hexw([plus("chrA", 100), 0, delim]).upper()))
    complete_only = line("g_far", 0, "chrA", 101, site, [plus("chrA", 100), 0, delim, plus("chrA", 900), 4, delim,
                                                         minus("chrA", 1000), 5, delim, plus("chrB", 200), 6, delim])
    # FASTA: another order than @SQ, one record more, chrB shorter than its LN
    def fa(names):
        out = []
        for k in names:
            s = text[k] if k in text else "ACGTTGCA" * 20
            out.append(f">{k} hand made\n" + "\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
        return "".join(out)

    fasta = fa(["chrC", "extra", "chrA", "chrB"])
    cases = {"hand": (head + "".join(good), fasta),
             "hand_far": (head + good[0] + complete_only, fasta)}
    # the raising kinds, one file each (a good record first: the error names the second record)
    hx = hexw([plus("chrA", 100), 0, delim])
    raising = {
        "raise_pam": line("r", 0, "chrA", 801, guide + "ANG", [plus("chrA", 800), 0, delim]),
        "raise_word": line("r", 0, "chrA", 101, site, [total, 0, delim]),
        "raise_word_neg": line("r", 0, "chrA", 101, site, [-total, 0, delim]),
        "raise_distance": line("r", 0, "chrA", 101, site, [plus("chrA", 100), 0, delim, plus("chrA", 900), 4, delim]),
        "raise_hex_odd": line("r", 0, "chrA", 101, site, None, "\tof:H:" + hx[:-1]),
        "raise_hex_half": line("r", 0, "chrA", 101, site, None, "\tof:H:" + hx + "01000000"),
        "raise_hex_digit": line("r", 0, "chrA", 101, site, None, "\tof:H:" + hx[:20] + "g" + hx[21:]),
        "raise_leading_delim": line("r", 0, "chrA", 101, site, [delim, plus("chrA", 100), 0, delim]),
    }
    for k, v in raising.items():
        cases[k] = (head + good[0] + v, fasta)
    cases["raise_chromosome"] = (head + good[0] + line("r", 0, "chrA", 101, site, [plus("chrA", 100), 0, delim]), fa(["chrC", "chrB"]))
    # the first record's hits are on chrA too: with chrA missing the first record is the one named
    return cases


def main():
    if sys.version_info >= (3, 12):
        sys.exit("sum() over floats is compensated from Python 3.12 on: the goldens need the plain left fold")
    if not REF.exists():
        sys.exit("needs the reference tree (build container only)")
    ns = reference_functions()
    OUT.mkdir(parents=True, exist_ok=True)
    mm, pam = ns["mm_scores"], ns["pam_scores"]
    assert len(mm) == 240 and len(pam) == 16
    (OUT / "cfd_tables.json").write_text(json.dumps({"mm": {k: float(v) for k, v in sorted(mm.items())},
                                                     "pam": {k: float(v) for k, v in sorted(pam.items())}}, indent=0))
    manifest = {}
    for name in ("ref_m3_sam", "ref_m3_sam_nag", "ref_m3_sam_max2", "ref_m2_sam_succinct"):
        manifest["toy_" + name] = dict(sam=f"../toy/{name}.sam", fasta="../toy/toy.fa")
    for name, (sam, fasta) in hand_made().items():
        (OUT / f"{name}.sam").write_text(sam)
        fname = "hand.fa" if name != "raise_chromosome" else "hand_missing.fa"
        (OUT / fname).write_text(fasta)
        manifest[name] = dict(sam=f"{name}.sam", fasta=fname)
    for name, c in manifest.items():
        sam, fasta = (OUT / c["sam"]).read_text(), read_fasta(OUT / c["fasta"])
        for mode in ("succinct", "complete"):
            got = run_script(ns, sam, fasta, mode)
            if isinstance(got, dict):
                c[mode] = got
            else:
                (OUT / f"{name}.{mode}.csv").write_text(got)
                c[mode] = f"{name}.{mode}.csv"
            print(name, mode, got if isinstance(got, dict) else f"{got.count(chr(10)) - 1} rows")
    (OUT / "cases.json").write_text(json.dumps(manifest, indent=1) + "\n")
    hand = (OUT / "hand.complete.csv").read_text()
    assert "e-" in hand, "no value in exponent form"


if __name__ == "__main__":
    main()

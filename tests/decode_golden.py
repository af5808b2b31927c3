"""The decode fixtures (tests/golden/decode, written by tools/make_decode_goldens.py from the reference's own
scripts/decode_database.py) and the synthetic database the GPU tests compare with the model."""
import json
import struct
from functools import lru_cache
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
DIR = ROOT / "tests" / "golden" / "decode"
MODES = ("succinct", "complete")
decode = import_module("guidescan-cli_amd.decode")

CASES = json.loads((DIR / "cases.json").read_text())
TABLES = decode.cfd_tables(DIR / "cfd_tables.json")  # the reference's values: the model under test does not take the library's
GOOD = [(n, m) for n, c in sorted(CASES.items()) for m in MODES if isinstance(c[m], str)]
RAISING = [(n, m) for n, c in sorted(CASES.items()) for m in MODES if not isinstance(c[m], str)]


def paths(name):
    c = CASES[name]
    return DIR / c["sam"], DIR / c["fasta"]


def expected(name, mode):
    return (DIR / CASES[name][mode]).read_bytes()


@lru_cache(maxsize=None)
def loaded(name):
    """-> (sq, records, fasta records) of a case"""
    sam, fa = paths(name)
    sq, recs = decode.parse_sam(sam.read_text())
    return sq, recs, decode.parse_fasta_records(fa)


def golden_floats():
    """every CFD and specificity the goldens print"""
    out = set()
    for name, mode in GOOD:
        for row in expected(name, mode).decode().splitlines()[1:]:
            last = row.rsplit(",", 1)[1]
            if last:
                out.add(float(last))
    return sorted(out)


def hexw(words):
    return "".join(struct.pack("<q", int(w)).hex() for w in words)


FOLD = {"fold65": 65, "fold257": 257, "fold70001": 70_001}  # the records of synthetic() that observe the ordered fold
FOLD_GROUPS = (2, 0, 1, 0, 3, 0, 1)                          # their groups' distances, in list order


@lru_cache(maxsize=None)
def synthetic():
    """A 50 kb genome of three chromosomes and 3,000 records whose lists straddle the decoder's tile (64 slots),
    workgroup (256) and scan-block edges, with one of 70,001 off-targets; words over the whole valid range with the
    boundary values.  Every 23-symbol slice has a PAM pair in A,C,G,T (no N in the genome): nothing raises.

    The boundary words give slices shorter than 23 symbols, so the records that hold them have no CFD sum.  The three
    FOLD records are there for the sum: 65, 257 and 70,001 off-targets, every one a planted near-copy of the record's
    own guide well inside s3 (a 23-symbol slice and a CFD up to 1.0 each, so the sum is large enough for the order of
    the additions to reach the printed digits), in groups of distances 2,0,1,0,3,0,1: the first distance-0 off-target
    stands in the middle of a 64-word chunk, behind the first chunk where the list is long enough, and further
    distance-0 groups follow in later chunks.  -> (sq, records, fasta records)"""
    rng = np.random.default_rng(2024)
    lens = [21_000, 17_003, 12_000]
    names = ["s1", "s2", "s3"]
    chrom = ["".join(rng.choice(list("ACGTacgt"), n, p=[.22, .22, .22, .22, .03, .03, .03, .03])) for n in lens]
    cum = np.cumsum([0] + lens)
    # 96 near-copies of a 20-mer + NGG in s3 from 5,000 on, every other one reverse-complemented (a '-' off-target)
    template = "".join(rng.choice(list("ACGT"), 20)) + "TGG"
    planted, at, s3 = [], 5_000, list(chrom[2])
    for j in range(96):
        copy = list(template)
        for i in rng.choice(20, int(rng.integers(0, 4)), replace=False):
            copy[i] = str(rng.choice([b for b in "ACGT" if b != copy[i]]))
        copy[20] = str(rng.choice(list("ACGT")))
        copy[21:23] = list(str(rng.choice(["GG", "GG", "GG", "AG", "GA", "CG"])))
        copy = "".join(copy)
        s3[at:at + 23] = copy if j % 2 == 0 else decode.revcom(copy)
        planted.append(int(cum[2]) + at + 22 if j % 2 == 0 else -(int(cum[2]) + at))
        at += 23 + int(rng.integers(0, 9))
    chrom[2] = "".join(s3)
    fasta = dict(zip(names, chrom))
    fasta["s2"] = fasta["s2"][:16_990]      # shorter than its LN
    sq = list(zip(names, lens))
    total = sum(lens)
    delim = -(total + 1)
    boundary = [0, 1, -1, total - 1, -(total - 1)]
    for c in cum[1:-1]:
        boundary += [int(c), -int(c), int(c) - 1, -(int(c) - 1), int(c) + 22, -(int(c) - 23), int(c) + 21]
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 70_001] + [int(x) for x in rng.integers(0, 40, 2988)] + list(FOLD.values())
    fold_at = dict(zip(range(len(sizes) - len(FOLD), len(sizes)), FOLD))
    order = rng.permutation(len(sizes))
    recs = []
    for k in order:
        n = sizes[k]
        if k in fold_at:
            words = rng.choice(planted, n).tolist()
            first = min(100, n // 3)        # the first distance-0 off-target is word first + 2 of the list
            words[0], words[first] = planted[0], planted[1]
            cuts = [first] + sorted(rng.choice(np.arange(first + 1, n), len(FOLD_GROUPS) - 2, replace=False).tolist())
            lst, at = [], 0
            for d, cut in zip(FOLD_GROUPS, cuts + [n]):
                lst += words[at:cut] + [d, delim]
                at = cut
            recs.append(decode.Record(fold_at[k], template, False, "s3", 4_000, hexw(lst)))
            continue
        words = rng.integers(-(total - 1), total, n).tolist()
        if n >= 63:
            words[:len(boundary)] = boundary
        # groups for distances 0..3 in order, some of them empty
        cuts = sorted(rng.integers(0, n + 1, 3).tolist())
        lst, at = [], 0
        for d, cut in enumerate(cuts + [n]):
            lst += words[at:cut] + [d, delim]
            at = cut
        ln = 23 if k % 11 else (20, 24, 21)[k % 3]
        c = int(rng.integers(0, 3))
        p = int(rng.integers(0, lens[c] - 24))
        seq = chrom[c][p:p + ln].upper()
        rev = bool(k % 5 == 0)
        hexs = None if k % 97 == 3 else hexw(lst)
        recs.append(decode.Record(f"syn{k}", seq, rev, names[c], p, hexs))
    return sq, recs, fasta


def tiny_bam(header_text, refs, records):
    """the bytes of a BAM file (SAMv1 section 4) in one gzip member and without the BGZF end-of-file block.
    refs = [(name, length)] of the binary reference list, records = [(refID, pos, flag, name, seq, of-hex or None)]"""
    import gzip
    out = b"BAM\1" + struct.pack("<i", len(header_text)) + header_text.encode() + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    for ref_id, pos, flag, name, seq, hexs in records:
        packed = bytearray((len(seq) + 1) // 2)
        for i, c in enumerate(seq):
            packed[i >> 1] |= "=ACMGRSVTWYHKDBN".index(c) << (0 if i & 1 else 4)
        body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, 0, 4680, 0, flag, len(seq), -1, -1, 0)
        body += name.encode() + b"\0" + bytes(packed) + b"\xff" * len(seq)
        if hexs is not None:
            body += b"ofH" + hexs.encode() + b"\0"
        out += struct.pack("<i", len(body)) + body
    return gzip.compress(out)

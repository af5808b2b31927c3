"""The rule of `--annotate`, restated in plain Python for tests/test_annot_model.py (host, no GPU), tests/test_gpu_annotate.py
and tests/test_cli_annotate_gpu.py: a double loop over printed rows and raw BED lines.  No segment table, no merging, no
code shared with the library or the reference.

A printed row whose match_position is s occupies the forward-strand bases [s - 1, s - 1 + L + P) of its chromosome, clipped
to [0, chromosome length); it has feature g iff that footprint shares a base with a BED line of group g on the chromosome.
Groups are numbered by first appearance; a row's features are distinct and ascend.  A hit that the position rule drops has
no row."""
import numpy as np


def bed_lines(bed):
    """-> (group names in order of first appearance, [(chromosome name, start, end, group number)] line by line)"""
    if isinstance(bed, bytes):
        bed = bed.decode()
    names, lines = [], []
    for line in bed.split("\n"):
        line = line.rstrip("\r")
        if not line or line[0] == "#" or line.startswith("track") or line.startswith("browser"):
            continue
        f = line.replace("\t", " ").split()
        name = f[3] if len(f) > 3 else f"{f[0]}:{f[1]}-{f[2]}"
        if name not in names:
            names.append(name)
        lines.append((f[0], int(f[1]), int(f[2]), names.index(name)))
    return names, lines


def resolve(pos, lengths, L, P):
    """a hit's signed absolute coordinate -> (chromosome, match_position, strand), or None where the row is dropped"""
    strand = "+"
    if pos < 0:
        pos, strand = -pos, "-"
    for c, n in enumerate(lengths):
        if pos < n:
            break
        pos -= n
    else:
        return None
    if strand == "+":
        e = pos + 1
        s = e - L - P + 1
    else:
        s = pos + 1
        e = s + L + P - 1
    if s < 0 or e > lengths[c]:
        return None
    return c, s, strand


def row_features(chr_name, s, w, chr_len, lines):
    """the ascending distinct group numbers of the row printed at s on chr_name"""
    lo, hi = max(s - 1, 0), min(s - 1 + w, chr_len)
    out = set()
    if lo < hi:
        for name, a, b, g in lines:
            if name == chr_name and a < hi and b > lo:
                out.add(g)
    return sorted(out)


def annotate(offsets, hits, chr_names, lengths, L, P, mismatches, bed):
    """-> (feat_offsets uint64[n_hits + 1], feats uint32, guide_counts uint32[n, mismatches + 1]) of the hit list
    hits[offsets[0]:offsets[n]], as GenomeIndex.annotate returns them"""
    _, lines = bed_lines(bed)
    lines = {name: [x for x in lines if x[0] == name] for name in chr_names}   # (a row meets its chromosome's lines only)
    n = len(offsets) - 1
    first = int(offsets[0])
    foff, feats = [0], []
    counts = np.zeros((n, mismatches + 1), dtype=np.uint32)
    for g in range(n):
        for h in range(int(offsets[g]), int(offsets[g + 1])):
            d = int(hits[h]["key"]) >> 61
            loc = resolve(int(hits[h]["pos"]), lengths, L, P)
            got = row_features(chr_names[loc[0]], loc[1], L + P, lengths[loc[0]], lines[chr_names[loc[0]]]) if loc else []
            feats += got
            if got:
                counts[g, d] += 1
            assert len(foff) == h - first + 1
            foff.append(len(feats))
    return np.array(foff, dtype=np.uint64), np.array(feats, dtype=np.uint32), counts


def column(features, names):
    return ";".join(names[g] for g in features) if features else "NA"


def csv_column(text, chr_names, lengths, w, bed):
    """the match_features column the rows of a CSV without it should get, row by row (header excluded): from each row's own
    match_chrm and match_position"""
    names, lines = bed_lines(bed)
    out = []
    for row in text.decode().splitlines():
        f = row.split(",")
        if f[2] == "NA":
            out.append("NA")
        else:
            out.append(column(row_features(f[2], int(f[3]), w, lengths[chr_names.index(f[2])], lines), names))
    return out


def split_column(text):
    """a CSV with the column -> (the same text without it, the column row by row)"""
    body, col = [], []
    for row in text.decode().splitlines():
        head, _, tail = row.rpartition(",")
        body.append(head)
        col.append(tail)
    return ("\n".join(body) + "\n" if body else "").encode(), col

"""Guides for regions, restated in plain Python: the BED rules with str.split, candidates from kmers.find_all_kmers,
membership as a double loop, hits from the oracle, specificity from score_model.specificity_batch, selection with
sorted() on tuples.  Shares no code with the library (csrc/gs_regions_scan.h, csrc/gs_design.hip)."""
from importlib import import_module

import numpy as np

import oracle_lib as ol
import score_model as sm

kmers = import_module("guidescan-cli_amd.kmers")

REASONS = {
    "few": "fewer than three fields",
    "integer": "start or end is not a non-negative integer",
    "order": "start >= end",
    "chromosome": "no such chromosome in the genome structure",
    "beyond": "end beyond the chromosome's length",
    "comma": "group name contains ','",
    "long": "group name too long: an id could pass 254 bytes",
    "empty": "no interval in the file",
}
KINDS = {k: i + 1 for i, k in enumerate(("few", "integer", "order", "chromosome", "beyond", "comma", "long", "empty"))}


class BedError(Exception):
    def __init__(self, kind, line):
        self.kind, self.line = kind, line
        self.message = (f"regions file: {REASONS[kind]}" if kind == "empty" else f"regions line {line}: {REASONS[kind]}")
        super().__init__(self.message)


def _integer(s):
    return int(s) if s.isascii() and s.isdigit() and len(s) <= 18 else None


def parse_bed(raw: bytes, names, lengths, prefix=""):
    """-> (group names in order of first appearance, {(group, chromosome): merged [start, end) list})"""
    text = raw.decode("latin-1")
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    groups, ivs = [], {}
    longest = max((len(n) for n in names), default=0)
    for no, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        if line == "" or line.startswith(("#", "track", "browser")):
            continue
        f = [x for x in line.replace("\t", " ").split(" ") if x]
        if len(f) < 3:
            raise BedError("few", no)
        s, e = _integer(f[1]), _integer(f[2])
        if s is None or e is None:
            raise BedError("integer", no)
        if s >= e:
            raise BedError("order", no)
        if f[0] not in names:
            raise BedError("chromosome", no)
        c = list(names).index(f[0])
        if e > lengths[c]:
            raise BedError("beyond", no)
        name = f[3] if len(f) > 3 else f"{f[0]}:{f[1]}-{f[2]}"
        if "," in name:
            raise BedError("comma", no)
        if len(prefix) + len(name) + 1 + longest + 1 + 10 + 2 > 254:
            raise BedError("long", no)
        if name not in groups:
            groups.append(name)
        ivs.setdefault((groups.index(name), c), []).append((s, e))
    if not ivs:
        raise BedError("empty", 0)
    merged = {}
    for key, lst in ivs.items():
        out = []
        for s, e in sorted(lst):
            if out and s <= out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], e))
            else:
                out.append((s, e))
        merged[key] = out
    return groups, merged


def records(groups, merged, chromosomes, pam, k, start=False):
    """chromosomes: list of (chr index, bytes).  -> list of dict(group, chr, pos, sense, seq), one per (candidate,
    group) where the candidate's footprint [pos - 1, pos - 1 + k + P) lies inside an interval of the group"""
    w = k + len(pam)
    out = []
    for c, chrm in chromosomes:
        for seq, pos, sense in kmers.find_all_kmers(chrm, pam, k, start):
            for g in range(len(groups)):
                for s, e in merged.get((g, c), ()):
                    if s <= pos - 1 and pos - 1 + w <= e:
                        out.append({"group": g, "chr": c, "pos": pos, "sense": sense, "seq": seq})
    return out


_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def score(recs, oidx, lengths, pam, mismatches=3, alt_pams=(), start=False, threshold=-1):
    """adds spec (float32, the CSV rule, no cap on the off-targets) and eligible to every record"""
    L, P = (len(recs[0]["seq"]), len(pam)) if recs else (0, len(pam))
    opts = ol.make_opts(mismatches=mismatches, alt_pams=alt_pams, start=start)
    topts = ol.make_opts(mismatches=max(threshold, 0), alt_pams=alt_pams, start=start, threshold=threshold)
    cache = {}
    for r in recs:
        if r["seq"] not in cache:
            hits, _, raw = oidx.enumerate(r["seq"], pam, opts)
            d = np.array([h[1] for h in hits], dtype=np.int64)
            cfd = np.empty(len(hits), np.float32)
            perfect = np.zeros(len(hits), bool)
            for j, h in enumerate(hits):
                ms = h[3].translate(_COMP)
                hp = ms[20:23] if len(ms) >= 20 else ""
                cfd[j] = np.float32(ol.lib().gso_calculate_cfd(r["seq"].encode(), ms.encode(), hp.encode()))
                perfect[j] = h[1] == 0 and len(hp) == 3 and hp[1:3] == "GG"
            dropped = sm.dropped_batch(lengths, np.array([h[0] for h in hits], dtype=np.int64), L, P)
            ol.lib().gso_free(raw[0])
            spec = sm.specificity_batch(np.array([0, len(hits)]), d, cfd, dropped, perfect)[0]
            eligible = True
            if threshold > 0:
                th, _, traw = oidx.enumerate(r["seq"], pam, topts)
                eligible = th is not None
                if traw is not None:
                    ol.lib().gso_free(traw[0])
            cache[r["seq"]] = (np.float32(spec), eligible)
        r["spec"], r["eligible"] = cache[r["seq"]]
    return recs


def select(recs, per_region=None, min_specificity=None):
    """the records in output order, cut"""
    ranked = per_region is not None

    def key(r):
        return (r["group"], -float(r.get("spec", 0.0)) if ranked else 0.0, r["chr"], r["pos"], r["sense"] == "-")

    out, taken = [], {}
    for r in sorted(recs, key=key):
        if not r.get("eligible", True):
            continue
        if min_specificity is not None and not np.float32(r["spec"]) >= np.float32(min_specificity):
            continue
        if per_region is not None and taken.get(r["group"], 0) >= per_region:
            continue
        taken[r["group"]] = taken.get(r["group"], 0) + 1
        out.append(r)
    return out


def ids(sel, groups, names, prefix=""):
    return [f"{prefix}{groups[r['group']]}:{names[r['chr']]}:{r['pos']}:{r['sense']}" for r in sel]


def rows(sel, groups, names, pam, prefix=""):
    return "".join(f"{i},{r['seq']},{pam},{names[r['chr']]},{r['pos']},{r['sense']}\n"
                   for i, r in zip(ids(sel, groups, names, prefix), sel))


def arrays(sel, groups, names, pam, prefix=""):
    """what DeviceKmers.to_host / ids_to_host give for the selection"""
    idl = [i.encode() for i in ids(sel, groups, names, prefix)]
    off = np.zeros(len(sel) + 1, dtype=np.uint64)
    if sel:
        off[1:] = np.cumsum([len(i) for i in idl])
    return {"seqs": "".join(r["seq"] for r in sel).encode(), "pams": (pam * len(sel)).encode(),
            "pos": np.array([r["pos"] for r in sel], dtype=np.uint32),
            "sense_chars": np.frombuffer("".join(r["sense"] for r in sel).encode(), dtype=np.uint8),
            "ids": b"".join(idl), "id_off": off,
            "sense": np.array([r["sense"] == "+" for r in sel], dtype=np.uint8)}

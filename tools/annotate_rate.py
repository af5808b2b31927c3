#!/usr/bin/env python3
"""What `--annotate` costs on one GPU, next to the only way the join could be done before it existed:
  (kernel)   gs_annotate_device alone on a synthesized hit list of HITS hits at uniformly random places of the genome, in
             guides of 256: HIP events around the call, REPEATS repeats behind two warm-ups -> hits per second, min / median /
             max; the first 2^20 hits are held equal to the host model (gs_debug_annotate_host);
  (command)  the wall time of `guidescan enumerate --all-candidates --encoder gpu` (CSV, succinct) with --annotate and without
             it, alternating, CLI_REPEATS runs each; and the same command without --annotate by the binary of the parent commit
             when parent=PATH names one: every run of this commit against every run of the parent, and the medians apart by
             twice the larger spread before anything is called a difference;
  (join)     the first JOIN_ROWS rows of the un-annotated CSV joined against the same BED file in plain Python, once, for
             scale, with the time the whole file would take at that rate next to it, named as an extrapolation.
    python tools/annotate_rate.py [parent=PATH/TO/guidescan] [out=profiles/annotate_rate.json] [join=1] [hits=33554432]
The genome is bench.py's synthetic chr1-sized one; the annotation is generated: 2 x 10^4 gene-like intervals, each laid over
ten of the 2 x 10^5 exon-like intervals of 150 bases, every interval a group of its own.  No number is fixed in advance."""
import bisect
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
synth = import_module("guidescan-cli_amd.synth")
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
PAM, K, M = "NGG", 20, 3
GENES, EXONS_PER_GENE, EXON = 20_000, 10, 150
REPEATS, CLI_REPEATS, JOIN_ROWS = 10, 5, 5_000_000


def say(msg):
    print(f"[annotate_rate] {msg}", file=sys.stderr, flush=True)


def make_bed(name, length, seed=11):
    """-> (BED text, [(start, end, group name)] sorted by start): gene g spans its ten exons and the introns between them"""
    rng = np.random.default_rng(seed)
    slot = length // GENES
    rows = []
    for g in range(GENES):
        span = int(rng.integers((EXONS_PER_GENE + 2) * 2 * EXON, slot - 1000))
        a = g * slot + int(rng.integers(0, slot - span))
        starts = np.sort(rng.choice(np.arange(a, a + span - EXON, 2 * EXON), EXONS_PER_GENE, replace=False))
        rows.append((int(starts[0]), int(starts[-1]) + EXON, f"gene{g:05d}"))
        rows += [(int(s), int(s) + EXON, f"gene{g:05d}.e{j}") for j, s in enumerate(starts)]
    rows.sort()
    return "".join(f"{name}\t{a}\t{b}\t{n}\n" for a, b, n in rows), rows


def spread(v):
    return {"min": min(v), "median": statistics.median(v), "max": max(v), "runs": v}


def kernel_rate(api, torch, text, names, lengths, bed, n_hits):
    gs = api.make_genome_structure(names, lengths)
    say("index build (the handle; its tables are not read)")
    gidx = api.GenomeIndex.build(text, device=0)
    rg = api.Regions.parse(bed.encode(), gs)
    an = api.Annotation.build(rg, device=0)
    rg.close()
    rng = np.random.default_rng(5)
    hits = np.zeros(n_hits, dtype=api.HIT_DTYPE)
    pos = rng.integers(K + len(PAM), lengths[0], n_hits)
    hits["pos"] = np.where(rng.random(n_hits) < 0.5, pos, -(pos - K - len(PAM)))
    per = 256
    offsets = np.arange(0, n_hits + 1, per, dtype=np.uint64)
    d = (np.arange(n_hits, dtype=np.uint64) % np.uint64(per)) * np.uint64(M + 1) // np.uint64(per)
    hits["key"] = d << np.uint64(61)
    n = offsets.shape[0] - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_o, d_h = up(offsets), up(hits)
    torch.cuda.synchronize()
    ms = []
    with gidx.locked():
        for rep in range(REPEATS + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gidx.annotate_device(an, gs, n, K, len(PAM), M, d_o.data_ptr(), d_h.data_ptr())
            b.record()
            torch.cuda.synchronize()
            if rep >= 2:
                ms.append(a.elapsed_time(b))
    # the same answers as the host model, on the head of the list
    head = 1 << 20
    got = gidx.annotate(an, gs, offsets[:head // per + 1], hits[:head], K, len(PAM), M)
    want = api.annotate_host_model(an, gs, offsets[:head // per + 1], hits[:head], K, len(PAM), M)
    same = all(np.array_equal(x, y) for x, y in zip(got, want))
    info = an.info()
    with_feature = int((np.diff(got[0].astype(np.int64)) > 0).sum())
    gidx.set_annotation(None)
    an.close()
    gidx.close()
    return {"hits": n_hits, "guides": n, "table": info, "table_bytes": 4 * (2 * info["segments"] + info["entries"]),
            "hit_bytes_streamed": 16 * n_hits, "ms_events": spread(ms),
            "hits_per_second": {k: n_hits / (1e-3 * v) for k, v in (("min", max(ms)), ("median", statistics.median(ms)), ("max", min(ms)))},
            "head_equals_host_model": bool(same), "head_hits_with_a_feature": with_feature, "head_hits": head,
            "note": "the call's time between two events: two kernels, the scan, three small copies and their synchronisations"}


def cli_run(binary, prefix, out, bed=None):
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    t0 = time.perf_counter()
    r = subprocess.run([str(binary), "enumerate", str(prefix), "--all-candidates", "--encoder", "gpu", "-m", str(M), "--mode", "succinct",
                        "-o", str(out)] + (["--annotate", str(bed)] if bed else []), capture_output=True, text=True, env=env)
    s = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{binary}: exit {r.returncode}\n{r.stderr}")
    return s


def python_join(csv_path, rows):
    """every row of the CSV against the BED's intervals: bisect on the starts, then back while an interval can still reach
    the row (genes are at most one slot long) -> (seconds, rows, rows with a feature)"""
    starts = [a for a, _, _ in rows]
    longest = max(b - a for a, b, _ in rows)
    w = K + len(PAM)
    t0 = time.perf_counter()
    n = hit = 0
    with open(csv_path) as f:
        f.readline()
        for line in f:
            c = line.split(",", 4)
            n += 1
            if n > JOIN_ROWS:
                n -= 1
                break
            if c[2] == "NA":
                continue
            hi = int(c[3]) - 1 + w
            lo = max(hi - w, 0)   # the row printed at 0 is clipped
            i = bisect.bisect_left(starts, hi)
            feats = []
            while i > 0 and starts[i - 1] + longest > lo:
                i -= 1
                if rows[i][1] > lo:
                    feats.append(rows[i][2])
            hit += bool(feats)
    return time.perf_counter() - t0, n, hit


def differs(a, b):
    """medians apart by twice the larger spread"""
    return abs(statistics.median(a) - statistics.median(b)) > 2 * max(max(a) - min(a), max(b) - min(b))


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    out_path = Path(args.get("out", ROOT / "profiles" / "annotate_rate.json"))
    parent = args.get("parent")
    n_hits = int(args.get("hits", 1 << 25))
    import torch
    api = import_module("guidescan-cli_amd.api")
    torch.zeros(1, device="cuda")
    say("synthetic chr1-sized genome")
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    lengths = [int(x) for x in lengths]
    bed, rows = make_bed(names[0], lengths[0])
    res = {"workload": "chr1", "genome_bases": lengths[0], "genes": GENES, "exons": GENES * EXONS_PER_GENE, "exon_bases": EXON,
           "mismatches": M, "pam": PAM, "kmer_length": K}
    res["kernel"] = kernel_rate(api, torch, text, names, lengths, bed, n_hits)
    say(f"kernel: {res['kernel']['ms_events']}")
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_annot_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        (d / "a.bed").write_text(bed)
        runs = {"plain": [], "annotate": [], "parent": []}
        cli_run(CLI, d / "g", d / "warm.csv")   # the page cache, the code objects
        for rep in range(CLI_REPEATS):
            say(f"command, round {rep}")
            runs["plain"].append(cli_run(CLI, d / "g", d / "plain.csv"))
            runs["annotate"].append(cli_run(CLI, d / "g", d / "annot.csv", d / "a.bed"))
            if parent:
                runs["parent"].append(cli_run(parent, d / "g", d / "parent.csv"))
        cmd = {"plain_seconds": spread(runs["plain"]), "annotate_seconds": spread(runs["annotate"]),
               "plain_csv_bytes": (d / "plain.csv").stat().st_size, "annotate_csv_bytes": (d / "annot.csv").stat().st_size,
               "annotate_differs_from_plain": differs(runs["annotate"], runs["plain"])}
        if parent:
            cmd["parent_seconds"] = spread(runs["parent"])
            cmd["plain_slower_than_every_parent_run"] = min(runs["plain"]) > max(runs["parent"])
            cmd["plain_differs_from_parent"] = differs(runs["plain"], runs["parent"])
            cmd["same_bytes_as_parent"] = (d / "plain.csv").read_bytes() == (d / "parent.csv").read_bytes()
        else:
            cmd["parent_seconds"] = "not run"
        res["command"] = cmd
        if args.get("join", "1") != "0":
            say("joining the plain CSV against the BED in Python")
            s, n, hit = python_join(d / "plain.csv", rows)
            with open(d / "plain.csv", "rb") as f:
                total = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 26), b"")) - 1
            res["python_join"] = {"seconds": s, "rows": n, "rows_with_a_feature": hit, "rows_of_the_file": total,
                                  "seconds_for_the_file_extrapolated": s * total / max(n, 1)}
        else:
            res["python_join"] = "not run"
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

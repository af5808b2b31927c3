#!/usr/bin/env python3
"""What guide pairs for regions cost on one GPU, pass by pass, next to the only way the job could
be done before `--pairs` existed, on the setting of tools/design_rate.py (bench.py's synthetic chr1-sized genome, 2x10^5
intervals of 150 bases in 2x10^4 groups, -m 3):
  (pairs)    scan, restrict and score as there; then Design.pairs(max_span=400, per_region=5) five times: the tallies, the
             chunks, and the median milliseconds of each pass between events on the call's stream (gs_pairs_ms), with the
             host clock around the call;
  (baseline) the same join in Python over the `--regions` table with its specificities (Design.to_host): per group the
             records sorted by cut, a double loop that stops at max_span, sorted() on the rank tuple, the first five.  For
             orientation only, as the 50 s of DESIGN.md section 6: the pairs must be the device's;
  (regions)  with parent=DIR (a build of the parent commit: DIR/bin/guidescan beside DIR/libgsamd.so): the existing command
             `enumerate --all-candidates --regions BED --per-region 3` under both builds, five runs each in turn, medians
             and spreads of the wall clock: what factoring the selection's passes cost the command that uses them.
    python tools/pairs_rate.py [out=profiles/pairs_rate.json] [parent=DIR] [baseline=1] [intervals=200000] [groups=20000]
No number is promised."""
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
sys.path.insert(0, str(ROOT / "tools"))
synth = import_module("guidescan-cli_amd.synth")
design_rate = import_module("design_rate")
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
PAM, K, M, MAX_SPAN, MIN_SPAN, CUT_OFFSET, PER_REGION, RUNS = "NGG", 20, 3, 400, 1, 3, 5, 5


def say(msg):
    print(f"[pairs_rate] {msg}", file=sys.stderr, flush=True)


def python_join(host):
    """-> [(group, chr, pos_a, sense_a, pos_b, sense_b)] in result order, by loops over the records of each group"""
    order = np.lexsort((host["sense"] == ord("-"), host["pos"], host["chr"], host["group"]))
    group, chrom, pos, sense, spec, elig = (host[x][order].tolist() for x in ("group", "chr", "pos", "sense", "spec", "eligible"))
    out, lo, n = [], 0, len(group)
    while lo < n:
        hi = lo
        while hi < n and group[hi] == group[lo]:
            hi += 1
        recs = []
        for i in range(lo, hi):
            if not elig[i]:
                continue
            right = sense[i] == ord("+")   # no --start here
            q = pos[i] - 1
            recs.append((chrom[i], q + K - CUT_OFFSET if right else q + len(PAM) + CUT_OFFSET, sense[i] == ord("-"), spec[i], pos[i], sense[i]))
        recs.sort(key=lambda r: r[:3])
        found = []
        for x, a in enumerate(recs):
            for y in range(x + 1, len(recs)):
                b = recs[y]
                if b[0] != a[0] or b[1] - a[1] > MAX_SPAN:
                    break
                if b[1] - a[1] >= MIN_SPAN:
                    found.append((-min(a[3], b[3]), -max(a[3], b[3]), x, y))
        found.sort()
        for _, _, x, y in found[:PER_REGION]:
            a, b = recs[x], recs[y]
            out.append((group[lo], a[0], a[4], chr(a[5]), b[4], chr(b[5])))
        lo = hi
    return out


def pairs_run(api, torch, text, names, lengths, bed, baseline):
    gs = api.make_genome_structure(names, lengths)
    say("index build, scan, restrict, score (as tools/design_rate.py times them)")
    gidx = api.GenomeIndex.build(text, device=0)
    rg = api.Regions.parse(bed.encode(), gs)
    km = api.generate_kmers(np.asarray(text[:lengths[0]]), PAM, K)
    d = km.restrict(rg, 0)
    km.close()
    d.score(gidx, mismatches=M)
    res = {"records": d.info()[0]}
    ms, host_ms, last, chosen = [], [], None, None
    for run in range(RUNS + 1):   # the first run warms the allocator and rocPRIM's kernels up and is left out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        guides, pr = d.pairs("", MAX_SPAN, MIN_SPAN, CUT_OFFSET, "any", PER_REGION)
        torch.cuda.synchronize()
        if run:
            host_ms.append(1e3 * (time.perf_counter() - t0))
            ms.append(pr.ms())
        last = pr.last()
        if run == RUNS:
            got = pr.to_host()
            _, _, gpos, gsense = guides.to_host()
            chosen = [(int(g), int(c), int(gpos[a]), chr(gsense[a]), int(gpos[b]), chr(gsense[b]))
                      for g, c, a, b in zip(got["group"], got["chr"], got["a"], got["b"])]
            res["guides"] = guides.n
        guides.close()
        pr.close()
    res.update(last)
    res["pass_ms_events_median"] = {k: statistics.median(m[k] for m in ms) for k in ms[0]}
    res["pass_ms_events_min_max"] = {k: [min(m[k] for m in ms), max(m[k] for m in ms)] for k in ms[0]}
    res["device_ms_events_median"] = statistics.median(sum(m.values()) for m in ms)
    res["call_ms_host_clock_median"] = statistics.median(host_ms)
    res["call_ms_host_clock_min_max"] = [min(host_ms), max(host_ms)]
    out = {"pairs": res}
    if baseline:
        say("the same join in Python over the records' table")
        host = d.to_host()
        t0 = time.perf_counter()
        joined = python_join(host)
        out["baseline"] = {"python_join_seconds": time.perf_counter() - t0, "pairs": len(joined), "same_pairs": joined == chosen}
    else:
        out["baseline"] = "not run"
    for x in (d, rg, gidx):
        x.close()
    return out


def regions_command(text, names, lengths, bed, parent):
    """wall clock of `enumerate --all-candidates --regions BED --per-region 3` under this build and the parent's, in turn"""
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_pairs_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        (d / "r.bed").write_text(bed)
        env = dict(os.environ)
        env.pop("GS_ENCODER", None)
        builds = {"this": CLI, "parent": Path(parent) / "bin" / "guidescan"}
        secs, outputs = {k: [] for k in builds}, {}
        for run in range(RUNS + 1):   # the first run of each is a warm-up
            for name, cli in builds.items():
                out = d / f"{name}.csv"
                t0 = time.perf_counter()
                r = subprocess.run([str(cli), "enumerate", str(d / "g"), "--all-candidates", "--regions", str(d / "r.bed"), "--per-region", "3",
                                    "-m", str(M), "--encoder", "gpu", "--mode", "succinct", "-o", str(out)], capture_output=True, text=True, env=env)
                if r.returncode != 0:
                    raise SystemExit(f"{name}: exit {r.returncode}\n{r.stderr}")
                if run:
                    secs[name].append(time.perf_counter() - t0)
                outputs[name] = out.read_bytes()
                say(f"{name} run {run}: {time.perf_counter() - t0:.3f} s")
        return {"command": "enumerate --all-candidates --regions BED --per-region 3 -m 3 --encoder gpu --mode succinct", "runs": RUNS,
                "seconds": secs, "median_seconds": {k: statistics.median(v) for k, v in secs.items()},
                "min_max_seconds": {k: [min(v), max(v)] for k, v in secs.items()}, "same_bytes": outputs["this"] == outputs["parent"],
                "csv_bytes": len(outputs["this"])}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    out_path = Path(args.get("out", ROOT / "profiles" / "pairs_rate.json"))
    n_intervals, n_groups = int(args.get("intervals", 200_000)), int(args.get("groups", 20_000))
    import torch
    api = import_module("guidescan-cli_amd.api")
    torch.zeros(1, device="cuda")
    say("synthetic chr1-sized genome")
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    lengths = [int(x) for x in lengths]
    bed, _, _ = design_rate.make_bed(names[0], lengths[0], n_intervals, n_groups)
    res = {"workload": "chr1", "genome_bases": lengths[0], "intervals": n_intervals, "interval_bases": design_rate.WIDTH, "groups": n_groups,
           "max_span": MAX_SPAN, "min_span": MIN_SPAN, "cut_offset": CUT_OFFSET, "orientation": "any", "per_region": PER_REGION, "mismatches": M,
           "pam": PAM, "kmer_length": K, "runs": RUNS}
    res.update(pairs_run(api, torch, text, names, lengths, bed, args.get("baseline", "1") != "0"))
    res["regions_command"] = regions_command(text, names, lengths, bed, args["parent"]) if "parent" in args else "not run"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

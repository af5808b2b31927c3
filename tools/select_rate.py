#!/usr/bin/env python3
"""What library selection costs on one GPU, in the set-up of tools/design_rate.py: bench.py's
synthetic chr1-sized genome and a generated BED of `intervals` intervals of 150 bases in `groups` groups.
  (filter)    gs_kmers_filter over the chromosome's scan under --gc 40:70 --max-run 3 --exclude-motif TTTT --exclude-site
              CGTCTC: its three passes between stream events, the whole call by the host clock, candidates per second;
  (selection) gs_design_select with --per-region 5, without and with --min-spacing 20: the whole call, and k_ds_space alone
              between its events.  The specificities are seeded random numbers uploaded through Design.set_scores: the
              selection's cost does not depend on where they come from, and no index is built;
  (adverse)   a single group over the whole chromosome with --per-region 1024 and a D the group cannot satisfy, so one wave
              walks every record: once with D = the chromosome's length (the kept list holds one cut) and once with D =
              length / 900 (it grows to about nine hundred);
  (regions)   with parent=DIR (a build of the parent commit: DIR/bin/guidescan beside DIR/libgsamd.so): the unchanged
              command `enumerate --all-candidates --regions BED --per-region 3` under both builds, six runs each in turn, the
              first left out (tools/pairs_rate.py's protocol): medians, smallest and largest.
    python tools/select_rate.py [out=profiles/select_rate.json] [parent=DIR] [intervals=200000] [groups=20000]
Every timed call runs six times and the first is left out.  No number is promised."""
import json
import statistics
import sys
import time
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
synth = import_module("guidescan-cli_amd.synth")
design_rate = import_module("design_rate")
pairs_rate = import_module("pairs_rate")
PAM, K, RUNS = "NGG", 20, 5


def say(msg):
    print(f"[select_rate] {msg}", file=sys.stderr, flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def timed(torch, fn, keep=None):
    """fn RUNS + 1 times, the first left out -> (spread of the host clock in ms, spread of the events in ms, extras of `keep`)"""
    host, dev, extra = [], [], []
    for run in range(RUNS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if run:
            host.append(1e3 * (time.perf_counter() - t0))
            dev.append(a.elapsed_time(b))
            if keep:
                extra.append(keep(out))
        last = out if run == RUNS else None
        if run != RUNS and hasattr(out, "close"):
            out.close()
    return spread(host), spread(dev), extra, last


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    out_path = Path(args.get("out", ROOT / "profiles" / "select_rate.json"))
    n_intervals, n_groups = int(args.get("intervals", 200_000)), int(args.get("groups", 20_000))
    import torch
    api = import_module("guidescan-cli_amd.api")
    torch.zeros(1, device="cuda")
    say("synthetic chr1-sized genome")
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    lengths = [int(x) for x in lengths]
    bed, _, _ = design_rate.make_bed(names[0], lengths[0], n_intervals, n_groups)
    gs = api.make_genome_structure(names, lengths)
    res = {"workload": "chr1", "genome_bases": lengths[0], "intervals": n_intervals, "interval_bases": design_rate.WIDTH,
           "groups": n_groups, "pam": PAM, "kmer_length": K, "runs": RUNS, "protocol": "six runs, the first left out"}

    km = api.generate_kmers(np.asarray(text[:lengths[0]]), PAM, K)
    rule = api.SeqRule(gc=(40, 70), max_run=3, exclude_motifs=("TTTT",), exclude_sites=("CGTCTC",))
    say(f"{km.n} candidates; filter")
    host, dev, passes, kept = timed(torch, lambda: km.filter(rule), keep=lambda f: f.filter_ms)
    res["filter"] = {"rule": "--gc 40:70 --max-run 3 --exclude-motif TTTT --exclude-site CGTCTC", "candidates": km.n, "kept": kept.n,
                     "counts": kept.filter_counts, "call_ms_host_clock": host, "call_ms_events": dev,
                     "pass_ms_events_median": {p: statistics.median(x[p] for x in passes) for p in ("rule", "scan", "gather")},
                     "candidates_per_second_by_the_call": km.n / (1e-3 * host["median"]),
                     "candidates_per_second_by_the_passes": km.n / (1e-3 * sum(statistics.median(x[p] for x in passes) for p in ("rule", "scan", "gather")))}
    kept.close()

    rg = api.Regions.parse(bed.encode(), gs)
    d = km.restrict(rg, 0)
    records = d.info()[0]
    rng = np.random.default_rng(5)
    d.set_scores(rng.random(records, dtype=np.float32), (rng.random(records) > 0.1).astype(np.uint8))
    say(f"{records} records; selection")
    sel = {"records": records, "per_region": 5, "scores": "seeded random specificities, one record in ten not eligible (Design.set_scores)"}
    host, dev, _, last = timed(torch, lambda: d.select("", 5))
    sel["unspaced"] = {"call_ms_host_clock": host, "call_ms_events": dev, "guides": last.n}
    last.close()
    d.set_spacing(20)
    host, dev, space, last = timed(torch, lambda: d.select("", 5), keep=lambda _: d.space_ms())
    sel["min_spacing_20"] = {"call_ms_host_clock": host, "call_ms_events": dev, "k_ds_space_ms_events": spread(space), "guides": last.n,
                             **d.last_spacing()}
    last.close()
    res["selection"] = sel
    d.close()
    rg.close()

    say("one group over the whole chromosome")
    whole = api.Regions.parse(f"{names[0]}\t0\t{lengths[0]}\tall\n".encode(), gs)
    d = km.restrict(whole, 0)
    records = d.info()[0]
    d.set_scores(rng.random(records, dtype=np.float32))
    adverse = {"records": records, "per_region": 1024, "note": "one wave of 64 lanes walks every record of the group"}
    for name, spacing in (("kept_list_of_one", lengths[0]), ("kept_list_of_about_900", lengths[0] // 900)):
        d.set_spacing(spacing)
        host, dev, space, last = timed(torch, lambda: d.select("", 1024), keep=lambda _: d.space_ms())
        adverse[name] = {"min_spacing": spacing, "call_ms_host_clock": host, "k_ds_space_ms_events": spread(space), "guides": last.n,
                         **d.last_spacing()}
        last.close()
        say(f"{name}: k_ds_space {adverse[name]['k_ds_space_ms_events']['median']:.1f} ms")
    d.set_spacing(0)
    host, dev, _, last = timed(torch, lambda: d.select("", 1024))
    adverse["unspaced"] = {"call_ms_host_clock": host, "guides": last.n}
    last.close()
    res["adverse"] = adverse
    d.close()
    whole.close()
    km.close()

    res["regions_command"] = pairs_rate.regions_command(text, names, lengths, bed, args["parent"]) if "parent" in args else "not run"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

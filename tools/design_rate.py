#!/usr/bin/env python3
"""What guides for regions cost on one GPU, stage by stage, next to the only way the job could be
done before `--regions` existed:
  (design)   scan of the chromosome, restrict to the BED's intervals, the score phase, select plus ids, and the final pass
             (search, scoring and CSV text of the selected guides: gs_enumerate_text_device), each between two events on the
             default stream, with the host clock next to it;
  (baseline) `guidescan enumerate --all-candidates --encoder gpu` over the whole chromosome (CSV, succinct), then the rows
             filtered by coordinate and specificity and ranked per group in Python, as tests/design_model.py states the
             rules: the selected ids must be the design's.
    python tools/design_rate.py [baseline=1] [out=profiles/design_rate.json] [intervals=200000] [groups=20000]
The genome is bench.py's synthetic chr1-sized one; the BED is generated: `intervals` intervals of 150 bases in `groups`
groups, seeded; --per-region 6 --min-specificity 0.2 -m 3.  No ratio is promised; the score phase is the existing search."""
import json
import os
import shutil
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
PAM, K, M, PER_REGION, MIN_SPEC, WIDTH = "NGG", 20, 3, 6, 0.2, 150


def say(msg):
    print(f"[design_rate] {msg}", file=sys.stderr, flush=True)


def make_bed(name, length, n_intervals, n_groups, seed=7):
    """-> (BED text, starts, groups): intervals of WIDTH bases at seeded places, interval i in group i % n_groups"""
    rng = np.random.default_rng(seed)
    starts = np.sort(rng.integers(0, length - WIDTH, size=n_intervals))
    groups = rng.permutation(n_intervals) % n_groups
    text = "".join(f"{name}\t{s}\t{s + WIDTH}\tg{g:05d}\n" for s, g in zip(starts.tolist(), groups.tolist()))
    return text, starts, groups


class Stages:
    """milliseconds of each stage between two events on the default stream, and by the host clock around the call"""

    def __init__(self, torch):
        self.torch, self.ms, self.host_ms = torch, {}, {}

    def run(self, name, fn):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        self.torch.cuda.synchronize()
        self.host_ms[name] = self.host_ms.get(name, 0.0) + 1e3 * (time.perf_counter() - t0)
        self.ms[name] = self.ms.get(name, 0.0) + a.elapsed_time(b)
        return out


def design_run(api, torch, text, names, lengths, bed):
    gs = api.make_genome_structure(names, lengths)
    say("index build (not timed as a stage)")
    t0 = time.perf_counter()
    gidx = api.GenomeIndex.build(text, device=0)
    build_s = time.perf_counter() - t0
    rg = api.Regions.parse(bed.encode(), gs)
    st = Stages(torch)
    chrm = np.asarray(text[:lengths[0]])
    km = st.run("scan", lambda: api.generate_kmers(chrm, PAM, K))
    scanned = km.n
    d = st.run("restrict", lambda: km.restrict(rg, 0))
    km.close()
    records = d.info()[0]
    say(f"{scanned} candidates, {records} records; score phase")
    st.run("score_phase", lambda: d.score(gidx, mismatches=M))
    sel = st.run("select_and_ids", lambda: d.select("", PER_REGION, MIN_SPEC))
    last = d.last_select()
    say(f"{sel.n} guides selected; final pass")
    batch, out_bytes = 1 << 17, 0
    for lo in range(0, sel.n, batch):
        n = min(batch, sel.n - lo)
        out_bytes += len(st.run("final_pass", lambda: gidx.enumerate_text_device(
            sel.seqs_ptr + lo * K, n, K, sel.pams_ptr + lo * len(PAM), len(PAM), sel.ids_ptr, sel.id_offsets_ptr + 8 * lo,
            sel.sense_positive_ptr + lo, gs, mismatches=M, complete=False)))
    ids, off, _ = sel.ids_to_host()
    chosen = [ids[int(off[i]):int(off[i + 1])].decode() for i in range(sel.n)]
    for x in (sel, d, rg, gidx):
        x.close()
    return dict(index_build_s=build_s, candidates_scanned=scanned, records=records, guides_selected=len(chosen),
                groups_empty=last["groups_empty"], groups_short=last["groups_short"], final_pass_bytes=out_bytes,
                stage_ms_events=st.ms, stage_ms_host_clock=st.host_ms), chosen


def baseline_run(text, names, lengths, starts, groups, n_groups):
    """the parent's way: the whole chromosome's database, then a filter in Python"""
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_design_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        out = d / "all.csv"
        env = dict(os.environ)
        env.pop("GS_ENCODER", None)
        say("enumerate --all-candidates over the chromosome")
        t0 = time.perf_counter()
        r = subprocess.run([str(CLI), "enumerate", str(d / "g"), "--all-candidates", "--encoder", "gpu", "-m", str(M), "--mode", "succinct",
                            "-o", str(out)], capture_output=True, text=True, env=env)
        cli_s = time.perf_counter() - t0
        if r.returncode != 0:
            raise SystemExit(f"baseline: exit {r.returncode}\n{r.stderr}")
        size = out.stat().st_size
        say(f"{size} bytes of CSV; filtering in Python")
        t0 = time.perf_counter()
        w = K + len(PAM)
        best = {}   # (chromosome:position:sense) -> specificity: one row per hit, the guide's specificity on each
        with open(out) as f:
            header = f.readline().rstrip("\n").split(",")
            spec_col = header.index("specificity")
            for line in f:
                c = line.rstrip("\n").split(",")
                best.setdefault(c[0], float(np.float32(c[spec_col])))
        keyed = []
        for gid, spec in best.items():
            name, pos, sense = gid.rsplit(":", 2)
            q = int(pos) - 1
            i = int(np.searchsorted(starts, q, side="right"))
            while i > 0 and starts[i - 1] + WIDTH >= q + w:   # intervals of one width: their ends ascend with their starts
                i -= 1
                if spec >= np.float32(MIN_SPEC):
                    keyed.append((int(groups[i]), -spec, int(pos), sense == "-", f"g{int(groups[i]):05d}:{gid}"))
        keyed.sort()
        chosen, taken, seen = [], {}, set()
        for g, _, _, _, rid in keyed:
            if rid in seen:   # two intervals of one group over one site: merged, one record
                continue
            seen.add(rid)
            if taken.get(g, 0) < PER_REGION:
                taken[g] = taken.get(g, 0) + 1
                chosen.append(rid)
        filter_s = time.perf_counter() - t0
        return dict(cli_seconds=cli_s, csv_bytes=size, python_filter_seconds=filter_s, guides_selected=len(chosen),
                    note="the baseline's specificities are the CSV's six decimals: a guide within 5e-7 of the bound or of a "
                         "neighbour in rank may fall the other way"), chosen
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    baseline = (sys.argv[1] if len(sys.argv) > 1 else "1") not in ("0", "baseline=0")
    out_path = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "design_rate.json"
    n_intervals = int(sys.argv[3]) if len(sys.argv) > 3 else 200_000
    n_groups = int(sys.argv[4]) if len(sys.argv) > 4 else 20_000
    import torch
    api = import_module("guidescan-cli_amd.api")
    torch.zeros(1, device="cuda")
    say("synthetic chr1-sized genome")
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    lengths = [int(x) for x in lengths]
    bed, starts, groups = make_bed(names[0], lengths[0], n_intervals, n_groups)
    res = {"workload": "chr1", "genome_bases": lengths[0], "intervals": n_intervals, "interval_bases": WIDTH, "groups": n_groups,
           "per_region": PER_REGION, "min_specificity": MIN_SPEC, "mismatches": M, "pam": PAM, "kmer_length": K}
    res["design"], chosen = design_run(api, torch, text, names, lengths, bed)
    if baseline:
        res["baseline"], base_chosen = baseline_run(text, names, lengths, starts, groups, n_groups)
        res["same_guides"] = sorted(chosen) == sorted(base_chosen)   # the design orders groups by first appearance
        res["guides_in_one_only"] = len(set(chosen) ^ set(base_chosen))
    else:
        res["baseline"] = "not run"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

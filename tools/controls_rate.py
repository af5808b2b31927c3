#!/usr/bin/env python3
"""What `guidescan controls` costs on one GPU, on the synthetic chr1-sized and hg38-sized genomes the
other rate tools use: L = 20, NGG, N = 1,000 controls at -m 2 and -m 3, first on a handle without the derived tables,
then on one that holds them (GenomeIndex.prepare builds them ahead: the call itself builds none before it has searched
their break-even); at hg38 size also -m 3 -a NAG with --max-candidates 2^28, which the i.i.d. estimate expects to end
short - the answer to "how strict can a control be" - likewise without and with the tables of that PAM set.
composition_acceptance is arithmetic, not a measurement: the mean of exp(-sites) over the G+C content of a uniform
20-mer in a genome with the synthetic genomes' base frequencies.
Per case: the report's counts, the acceptance at each step against the i.i.d. estimate, the rounds, the milliseconds per
stage between stream events and the call by the host clock (one warm-up call, then the median of five with the range),
the candidates searched per second by the search stage; the search's own device time (gs_enumerate_device's ms_total) on
as many synth.sample_guides guides as the case searched and on the generator's own words, same handle, same run, at that
count and at a full round of 2^20; and the share of the stages that is not the search.
  (commands)  with parent=DIR (a build of the parent commit: DIR/bin/guidescan beside DIR/libgsamd.so): `enumerate -f` and
              `enumerate --all-candidates --regions BED --per-region 3` on a 5 Mbp genome under both builds, compared byte
              for byte: neither runs new code.
    python tools/controls_rate.py [out=profiles/controls_rate.json] [sizes=chr1,hg38] [parent=DIR] [n=1000]
No number is promised."""
import json
import math
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
PAM, L, RUNS, SEED = "NGG", 20, 5, 1
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"


def say(msg):
    print(f"[controls_rate] {msg}", file=sys.stderr, flush=True)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def iid_sites(bases, m, n_alt=0):
    """sites a random 20-mer expects within m mismatches in an i.i.d. uniform genome: both strands, NGG (+ alt PAMs)"""
    ball = sum(math.comb(L, d) * 3 ** d for d in range(m + 1))
    return 2.0 * bases * (1 + n_alt) / 16.0 * ball / 4.0 ** L


def composition_acceptance(bases, m, alt=False, pg=0.21, pa=0.29, non_n=0.975):
    """mean over the G+C content k of a uniform L-mer of exp(-sites(k)): a letter matches a genome base with probability pg
    (G, C) or pa (A, T); 2 * non-N bases * pg^2 NGG sites on the two strands, pg * pa more for NAG"""
    sites = 2.0 * bases * non_n * (pg * pg + (pg * pa if alt else 0.0))
    acc = 0.0
    for k in range(L + 1):
        p = sum(math.comb(k, a) * (1 - pg) ** a * pg ** (k - a) * math.comb(L - k, b) * (1 - pa) ** b * pa ** (L - k - b)
                for a in range(min(k, m) + 1) for b in range(min(L - k, m - a) + 1))
        acc += math.comb(L, k) / 2.0 ** L * math.exp(-sites * p)
    return acc


def case(api, index, bases, n, m, alt=(), tables=False, max_candidates=1 << 32, runs=RUNS):
    no_new_tables = not tables
    if tables:      # the handle builds the tables of this shape ahead of the timed calls
        index.prepare(1000, L=L, pam=PAM, alt_pams=alt, mismatches=m)
    host, stages, rep = [], [], None
    for run in range(runs + 1):                         # the first call is the warm-up
        t0 = time.perf_counter()
        km, rep = api.controls(index, n, L=L, pam=PAM, seed=SEED, mismatches=m, alt_pams=alt, no_new_tables=no_new_tables,
                               max_candidates=max_candidates)
        km.close()
        if run:
            host.append(1e3 * (time.perf_counter() - t0))
            stages.append(rep["ms"])
    names = api.CONTROLS_STAGES
    med = {s: statistics.median(x[s] for x in stages) for s in names}
    searched = rep["looked_at"] - rep["gc"] - rep["run"] - rep["motif"]
    total = sum(med.values())
    sites = iid_sites(bases, m, len(alt))
    out = {"mismatches": m, "alt_pams": list(alt), "derived_tables": not no_new_tables, "max_candidates": max_candidates, "timed_calls": len(host),
           "report": {k: rep[k] for k in api.CONTROLS_COUNTS},
           "acceptance": {"search": (searched - rep["targeting"]) / searched if searched else None,
                          "distance": rep["kept"] / (rep["kept"] + rep["close"]) if rep["kept"] + rep["close"] else None,
                          "overall": rep["kept"] / rep["looked_at"] if rep["looked_at"] else None,
                          "iid_expected_sites": sites, "iid_search_acceptance": math.exp(-sites),
                          "composition_search_acceptance": composition_acceptance(bases, m, bool(alt))},
           "stage_ms": {s: spread([x[s] for x in stages]) for s in names}, "call_ms_host_clock": spread(host),
           "searched": searched, "searched_per_second_by_the_search_stage": searched / (1e-3 * med["search"]) if med["search"] else None,
           "share_not_search": (total - med["search"]) / total if total else None,
           "largest_other_stage": max((s for s in names if s != "search"), key=lambda s: med[s])}
    say(f"m={m} alt={alt} tables={not no_new_tables}: kept {rep['kept']} of {rep['looked_at']}, {rep['rounds']} round(s), "
        f"call {out['call_ms_host_clock']['median']:.1f} ms, search {med['search']:.1f} ms")
    return out


def search_alone(torch, api, index, text, count, m):
    """the search's own rate on `count` guides, once genome samples and once the generator's first `count` words (what a
    round searches): ms_total of gs_enumerate_device - device time, no host side - median of RUNS after a warm-up"""
    out = {"guides": count, "mismatches": m}
    pams = np.tile(np.frombuffer(PAM.encode(), dtype=np.uint8), (count, 1))
    for name, seqs in (("genome_samples", synth.sample_guides(text, count, seed=4242)[0]), ("random_words", api.control_sequences(SEED, 0, count, L))):
        d_s, d_p = torch.from_numpy(np.ascontiguousarray(seqs)).cuda(), torch.from_numpy(np.ascontiguousarray(pams)).cuda()
        ms = []
        for run in range(RUNS + 1):
            _, _, stats = index.enumerate_device(d_s.data_ptr(), count, L, d_p.data_ptr(), 3, mismatches=m)
            torch.cuda.synchronize()
            if run:
                ms.append(stats["ms_total"])
        out[name] = {"ms_total": spread(ms), "guides_per_second": count / (1e-3 * statistics.median(ms))}
    out["random_over_samples_ms"] = out["random_words"]["ms_total"]["median"] / out["genome_samples"]["ms_total"]["median"]
    return out


def unchanged_commands(parent):
    """the two existing commands under this build and the parent's on one 5 Mbp genome: same bytes?"""
    design_rate = import_module("design_rate")
    text, names, lengths = synth.make_genome([3_000_000, 2_000_000], seed=9)
    lengths = [int(x) for x in lengths]
    seqs, pams, pos, strands = synth.sample_guides(text, 2000, seed=5)
    bed, _, _ = design_rate.make_bed(names[0], lengths[0], 2000, 400)
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_controls_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        (d / "r.bed").write_text(bed)
        sq = [x.decode() for x in np.ascontiguousarray(seqs).view(f"S{seqs.shape[1]}").ravel()]
        (d / "k.csv").write_text("id,sequence,pam,chromosome,position,sense\n" +
                                 "".join(f"g{i},{sq[i]},NGG,{names[0]},{int(pos[i]) + 1},{chr(strands[i])}\n" for i in range(len(sq))))
        env = dict(os.environ)
        env.pop("GS_ENCODER", None)
        commands = {"enumerate -f": ["-f", str(d / "k.csv"), "-m", "3"],
                    "enumerate --all-candidates --regions BED --per-region 3": ["--all-candidates", "--regions", str(d / "r.bed"), "--per-region", "3", "-m", "3"]}
        res = {}
        for name, args in commands.items():
            outs = {}
            for build, cli in (("this", CLI), ("parent", Path(parent) / "bin" / "guidescan")):
                out = d / f"{build}.csv"
                r = subprocess.run([str(cli), "enumerate", str(d / "g")] + args + ["-o", str(out)], capture_output=True, text=True, env=env, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"{build} {name}: exit {r.returncode}\n{r.stderr}")
                outs[build] = out.read_bytes()
            res[name] = {"same_bytes": outs["this"] == outs["parent"], "bytes": len(outs["this"])}
            say(f"{name}: same bytes {res[name]['same_bytes']} ({res[name]['bytes']} B)")
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    out_path = Path(args.get("out", ROOT / "profiles" / "controls_rate.json"))
    sizes, n = args.get("sizes", "chr1,hg38").split(","), int(args.get("n", 1000))
    import torch
    api = import_module("guidescan-cli_amd.api")
    torch.zeros(1, device="cuda")
    res = {"pam": PAM, "kmer_length": L, "n": n, "seed": SEED, "round": api.controls_round(), "runs": RUNS,
           "protocol": "one warm-up call, then the median of five with the smallest and largest; the cases without the derived tables run "
                       "first, on a handle that has built none",
           "iid_note": "the estimate is for uniform i.i.d. bases; the synthetic genomes draw A,T at 0.29 and C,G at 0.21 and hold N blocks",
           "workloads": {}}
    for size in sizes:
        lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS}[size]
        say(f"synthetic {size}-sized genome")
        text, names, lengths = synth.make_genome(lengths, seed=1)
        bases = int(sum(int(x) for x in lengths))
        t0 = time.perf_counter()
        index = api.GenomeIndex.build(text, device=0)
        w = {"genome_bases": bases, "index_build_s": time.perf_counter() - t0, "cases": [], "search_alone": []}
        for tables in (False, True):
            for m in (2, 3):
                w["cases"].append(case(api, index, bases, n, m, tables=tables))
        for m in (2, 3):
            count = min(api.controls_round(), max(c["searched"] for c in w["cases"] if c["mismatches"] == m))
            w["search_alone"].append(search_alone(torch, api, index, text, count, m))
            w["search_alone"].append(search_alone(torch, api, index, text, api.controls_round(), m))
        if size == "hg38":
            w["strict"] = [case(api, index, bases, n, 3, alt=("NAG",), tables=t, max_candidates=1 << 28, runs=2) for t in (False, True)]
        index.close()
        del text
        res["workloads"][size] = w
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1) + "\n")       # what is measured so far survives a later stop
    res["existing_commands"] = unchanged_commands(args["parent"]) if "parent" in args else "not run"
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

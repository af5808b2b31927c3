#!/usr/bin/env python3
"""What reading the kmers file of `guidescan enumerate -f` costs, on the host and on the device (gs_kmersfile.hip,
`--kmers host|gpu`), on one GPU, recorded in profiles/kmers_file_rate.json - a record, not a threshold.  Two kmers files
on the synthetic genome of bench.py at the given size:
  rows_1m   1,000,000 sampled NGG 20-mers, the shape of bench.py's end-to-end row;
  chr21     every candidate of the genome's chr21 as `guidescan kmers --chromosomes chr21` writes them.
Each is enumerated (-m 3, CSV, --encoder gpu, 16 formatting threads) with --kmers host and --kmers gpu alternating, after
one run of each that is not counted (page cache, device); two counted runs each, both reported:
  (a) the seconds of cli::read_kmers, from the host path's --verbose stage line (the parent's behaviour in this binary);
  (b) the three times of the gpu stage line: file reads, waits for the uploads, the device stage;
  (c) the wall time of the whole command and its seconds after the index load, with the SHA-256 of the output, which must
      be one value over all runs of a file;
  (d) the peak resident host memory of the command (ru_maxrss of the child);
  (e) gs_kmers_parse_file called in this process, where the device is already up: after one call that is not counted, three
      calls with the report's milliseconds - the host clocks of (b) and the passes alone, by events in the stream.
    python tools/kmers_file_rate.py [workload=hg38] [out=profiles/kmers_file_rate.json] [passes]
With `passes` only (e) is taken and merged into the file that is there: the commands of (a)-(d) take minutes."""
import hashlib
import json
import os
import re
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
api = import_module("guidescan-cli_amd.api")
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
RUNS = 2
THREADS = 16


def note(msg):
    print(f"[kmers_file_rate] {msg}", file=sys.stderr, flush=True)


def run_cli(args, env):
    """-> (stdout, wall seconds)"""
    t0 = time.perf_counter()
    p = subprocess.Popen([str(CLI)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    out, err = p.communicate(timeout=1500)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(f"{args}: status {p.returncode}: {err[-400:]}")
    return out, wall


def run_measured(args, env):
    """-> (stdout and stderr, wall seconds, peak resident bytes of the child): wait4 hands back the child's own rusage"""
    t0 = time.perf_counter()
    log = tempfile.TemporaryFile(mode="w+")
    p = subprocess.Popen([str(CLI)] + [str(a) for a in args], stdout=log, stderr=subprocess.STDOUT, text=True, env=env)
    _, status, ru = os.wait4(p.pid, 0)
    p.returncode = os.waitstatus_to_exitcode(status)
    wall = time.perf_counter() - t0
    log.seek(0)
    out = log.read()
    log.close()
    if p.returncode != 0:
        raise RuntimeError(f"{args}: status {p.returncode}: {out[-400:]}")
    return out, wall, ru.ru_maxrss * 1024


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def measure(d, kmers, env):
    res = {"kmers_file_bytes": kmers.stat().st_size, "host": [], "gpu": []}
    order = ["host", "gpu"] + ["host", "gpu"] * RUNS          # the first pair is not counted
    for i, who in enumerate(order):
        o = d / "o.csv"
        if o.exists():
            o.unlink()
        out, wall, rss = run_measured(["enumerate", d / "g", "-f", kmers, "-o", o, "-m", "3", "--encoder", "gpu", "-n", THREADS,
                                       "--kmers", who, "--verbose"], env)
        if i < 2:
            continue
        e = {"wall_s": wall, "peak_resident_bytes": rss, "output_bytes": o.stat().st_size, "sha256": sha256(o),
             "seconds_after_index_load": float(re.search(r"Processed \d+ kmers in ([0-9.eE+-]+) seconds", out).group(1)),
             "rows": int(re.search(r"Read in (\d+) kmer", out).group(1))}
        if who == "host":
            e["read_kmers_s"] = float(re.search(r"kmers host: read_kmers ([0-9.eE+-]+) s", out).group(1))
        else:
            m = re.search(r"kmers gpu: file reads ([0-9.eE+-]+) s, waits for the uploads ([0-9.eE+-]+) s, device stage ([0-9.eE+-]+) s", out)
            e["file_reads_s"], e["upload_waits_s"], e["device_stage_s"] = (float(x) for x in m.groups())
            e["reader_s"] = e["file_reads_s"] + e["upload_waits_s"] + e["device_stage_s"]
            m = re.search(r"Encoder: gpu \((\d+) batch\(es\) encoded on the device, (\d+) by the host encoders\)", out)
            e["batches_on_device"], e["batches_on_host"] = int(m.group(1)), int(m.group(2))
        res[who].append(e)
        note(f"{kmers.name} --kmers {who}: wall {wall:.2f} s, " + (f"read_kmers {e['read_kmers_s']:.3f} s" if who == "host"
                                                                  else f"reader {e['reader_s']:.3f} s"))
    res["outputs_identical"] = len({e["sha256"] for w in ("host", "gpu") for e in res[w]}) == 1
    return res


def in_process(kmers):
    runs = []
    for i in range(4):
        t0 = time.perf_counter()
        km = api.DeviceKmers.parse(kmers)
        wall = time.perf_counter() - t0
        if i:
            runs.append(dict(wall_ms=wall * 1e3, rows=km.n, **{k + "_ms": v for k, v in km.report["ms"].items()}))
        km.close()
    size = kmers.stat().st_size
    for r in runs:
        r["passes_ms"] = sum(r[k + "_ms"] for k in ("summaries", "line_starts", "line_walk", "row_scan", "emit"))
        r["file_GB_per_s_over_the_passes"] = size / (r["passes_ms"] * 1e-3) / 1e9
    return runs


def main():
    workload = sys.argv[1] if len(sys.argv) > 1 else "hg38"
    out_path = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "kmers_file_rate.json"
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[workload]
    passes_only = len(sys.argv) > 3 and sys.argv[3] == "passes"
    n = 1_000_000
    text, names, lengths = synth.make_genome(lengths, seed=1)
    seqs, pams, pos, strands = synth.sample_guides(text, n, seed=7777)
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_kmf_", dir=base))
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    res = {"workload": workload, "files_on": base, "runs": RUNS, "mismatches": 3, "format": "csv complete", "encoder": "gpu",
           "format_threads": THREADS}
    if passes_only:
        res = json.loads(out_path.read_text())
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        sq = [x.decode() for x in np.ascontiguousarray(seqs).view(f"S{seqs.shape[1]}").ravel()]
        (d / "k1m.csv").write_text("id,sequence,pam,chromosome,position,sense\n" +
                                   "".join(f"g{i},{sq[i]},NGG,chr1,{int(pos[i]) + 1},{chr(strands[i])}\n" for i in range(n)))
        del text, seqs, sq
        note("genome and the 1 M-row file written")
        chrom = names[20] if len(names) > 20 else names[-1]
        run_cli(["kmers", d / "g", "-o", d / "k21.csv", "--chromosomes", chrom], env)
        if not passes_only:
            res["rows_1m"] = measure(d, d / "k1m.csv", env)
            res["chr21"] = dict(chromosome=chrom, **measure(d, d / "k21.csv", env))
        res["rows_1m"]["e_in_process"] = in_process(d / "k1m.csv")
        res["chr21"]["e_in_process"] = in_process(d / "k21.csv")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: (v if not isinstance(v, dict) else {"outputs_identical": v["outputs_identical"], "e_in_process": v["e_in_process"]})
                      for k, v in res.items()}))


if __name__ == "__main__":
    main()

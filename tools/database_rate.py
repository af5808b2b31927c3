#!/usr/bin/env python3
"""What the candidate database of one chromosome costs, end to end, the old way and the new one, on one GPU:
  (a) the way before `guidescan kmers` / `enumerate --all-candidates` existed: the candidates scanned on the device, their
      kmers-file rows formatted row by row in Python (what kmers.write_kmers_csv(device=D) did then; restated here, since it
      encodes the rows on the device now), then `guidescan enumerate -f KMERS --encoder gpu`;
  (b) `guidescan kmers` alone, and `guidescan enumerate --all-candidates --encoder gpu`.
Wall time of every step, the CLI's own stage lines, the candidate count, the bytes written and the SHA-256 of each output:
(a)'s and (b)'s files must be the same file.  Two runs of every row, both reported.
    python tools/database_rate.py [workload=hg38] [chromosome=chr21] [out=profiles/database_rate.json]
The genome is bench.py's synthetic one of that size (chr21: 46.7 Mbp, the chromosome BASELINE config 4's small form uses);
-m 3, CSV succinct and SAM complete, every file in /dev/shm."""
import hashlib
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
kmers = import_module("guidescan-cli_amd.kmers")
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
FORMATS = {"csv_succinct": ["--format", "csv", "--mode", "succinct"], "sam_complete": ["--format", "sam", "--mode", "complete"]}
RUNS = 2


def sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def say(msg):
    print(f"[database_rate] {msg}", file=sys.stderr, flush=True)


def cli(args):
    """-> (wall seconds, stdout)"""
    say(" ".join(str(a) for a in args[:1] + args[2:]))
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    t0 = time.perf_counter()
    r = subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, env=env)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{args}: exit {r.returncode}\n{r.stderr}")
    return dt, r.stdout


def stage_lines(log):
    keep = ("Scanned ", "Built the forward", "Processed ", "Stages", "Candidates:", "Encoder:", "Wrote ")
    return [ln for ln in log.splitlines() if ln.startswith(keep)]


def rows_in_python(chrm, name, path):
    """the parent's kmers file: device scan, then one formatted row per candidate on the host"""
    say("rows in Python")
    t0 = time.perf_counter()
    found = kmers.find_all_kmers_device(chrm, "NGG", 20, False, 0)
    t1 = time.perf_counter()
    with open(path, "w") as fh:
        fh.write("id,sequence,pam,chromosome,position,sense\n")
        for kmer, pos, sense in found:
            fh.write(f"{name}:{pos}:{sense},{kmer},NGG,{name},{pos},{sense}\n")
    t2 = time.perf_counter()
    return dict(seconds=t2 - t0, scan_and_download_seconds=t1 - t0, format_and_write_seconds=t2 - t1, candidates=len(found))


def main():
    workload = sys.argv[1] if len(sys.argv) > 1 else "hg38"
    chrom = sys.argv[2] if len(sys.argv) > 2 else "chr21"
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "database_rate.json"
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[workload]
    say(f"synthetic genome, {sum(lengths)} bases")
    text, names, lengths = synth.make_genome(lengths, seed=1)
    c = names.index(chrom)
    begin = int(sum(lengths[:c]))
    chrm = np.asarray(text[begin:begin + lengths[c]])
    res = {"workload": workload, "chromosome": chrom, "chromosome_bases": lengths[c], "genome_bases": int(sum(lengths)),
           "mismatches": 3, "runs_per_row": RUNS, "kmers_file": {}, "database": {}}
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_db_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        del text
        # the kmers file: (a) rows formatted in Python, (b) `guidescan kmers`
        ka, kb = d / "a.kmers.csv", d / "b.kmers.csv"
        res["kmers_file"]["a_python_rows"] = [rows_in_python(chrm, chrom, ka) for _ in range(RUNS)]
        res["kmers_file"]["b_guidescan_kmers"] = []
        for _ in range(RUNS):
            dt, log = cli(["kmers", d / "g", "-o", kb, "--chromosomes", chrom])
            res["kmers_file"]["b_guidescan_kmers"].append(dict(seconds=dt, stages=stage_lines(log)))
        res["kmers_file"]["bytes"] = ka.stat().st_size
        res["kmers_file"]["sha256"] = {"a": sha256(ka), "b": sha256(kb)}
        res["candidates"] = res["kmers_file"]["a_python_rows"][0]["candidates"]
        kb.unlink()
        for fmt, opts in FORMATS.items():
            row = {"a_enumerate_f": [], "b_all_candidates": []}
            out = d / f"out.{fmt}"
            for key, source in (("a_enumerate_f", ["-f", ka]), ("b_all_candidates", ["--all-candidates", "--chromosomes", chrom])):
                for _ in range(RUNS):
                    dt, log = cli(["enumerate", d / "g", "-o", out, "-m", "3", "--encoder", "gpu"] + source + opts)
                    row[key].append(dict(seconds=dt, stages=stage_lines(log)))
                row.setdefault("bytes", out.stat().st_size)
                row.setdefault("sha256", {})[key[0]] = sha256(out)
                out.unlink()
            row["same_file"] = row["sha256"]["a"] == row["sha256"]["b"]
            kmers_a = [r["seconds"] for r in res["kmers_file"]["a_python_rows"]]
            row["a_total_seconds"] = [k + e["seconds"] for k, e in zip(kmers_a, row["a_enumerate_f"])]
            row["b_total_seconds"] = [e["seconds"] for e in row["b_all_candidates"]]
            res["database"][fmt] = row
        res["kmers_file"]["same_file"] = res["kmers_file"]["sha256"]["a"] == res["kmers_file"]["sha256"]["b"]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    ok = res["kmers_file"]["same_file"] and all(r["same_file"] for r in res["database"].values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

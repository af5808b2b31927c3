#!/usr/bin/env python3
"""What `guidescan decode --annotate` costs on one GPU, recorded in profiles/decode_annotate_rate.json -
a record, not a threshold.  The claim it checks: `decode` WITHOUT the option is within the parent commit's run-to-run spread.
  (command)  the wall time of `guidescan decode --mode complete --bgzf gpu -o OUT DB.bam GENOME.fa` without --annotate, with it,
             and - parent=PATH naming the parent commit's binary - by that binary without it: one warm-up each, then REPEATS
             rounds in which the three take turns; medians of the rounds with min and max; the medians apart by twice the
             larger spread before anything is called a difference; the un-annotated tables of both binaries compared byte for
             byte, and the annotated table without its last column against them;
  (pass)     the annotation pass alone (k_dc_feat: one lane per off-target word) between two stream events, as the decoder
             reports it (gs_debug_decode_annot_ms), in gs_decode_bam_device over the whole file as one call: REPEATS calls
             after the first, next to a host clock around the whole call with and without the flag.
    python tools/decode_annotate_rate.py [parent=PATH/TO/guidescan] [out=profiles/decode_annotate_rate.json] [guides=0]
The genome is bench.py's synthetic chr1-sized one and the BED file the one tools/annotate_rate.py synthesises (2 x 10^4 genes
over 2 x 10^5 exons).  The database is made here by `guidescan enumerate --all-candidates --format bam --bgzf gpu --mode complete
-m 3`; guides=N (for a rehearsal) takes the first N candidates of `guidescan kmers` instead.  No number is fixed in advance."""
import gzip
import json
import os
import shutil
import statistics
import struct
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
decode = import_module("guidescan-cli_amd.decode")
from annotate_rate import differs, make_bed, spread   # noqa: E402  (the BED shape and the spread rule of that record)

CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
M, REPEATS = 3, 5


def say(msg):
    print(f"[decode_annotate_rate] {msg}", file=sys.stderr, flush=True)


def run(cmd):
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    t0 = time.perf_counter()
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, env=env)
    s = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"{cmd[0]} {cmd[1]}: exit {r.returncode}\n{r.stderr[-600:]}")
    return s, (r.stderr.strip().splitlines() or [""])[0]


def decode_cmd(binary, db, fa, out, bed=None):
    return [binary, "decode", "--mode", "complete", "--bgzf", "gpu", "--verbose", "-o", out] + (["--annotate", bed] if bed else []) + [db, fa]


def same_without_last_column(annotated, plain):
    with open(annotated, "rb") as a, open(plain, "rb") as p:
        for la, lp in zip(a, p):
            if la.rsplit(b",", 1)[0] + b"\n" != lp:
                return False
        return a.readline() == b"" and p.readline() == b""


def pass_alone(db, fa, bed_path):
    """gs_decode_bam_device over the whole file as one call -> the record of the (pass) section"""
    api = import_module("guidescan-cli_amd.api")
    data = Path(db).read_bytes()
    sizes = decode.bgzf_member_sizes(data)
    head, n_head = b"", 0
    while True:
        try:
            sq, ref_to_sq, skip = decode.bam_header(head)
            break
        except (struct.error, ValueError, IndexError):
            at = sum(sizes[:n_head])
            head += gzip.decompress(data[at:at + sizes[n_head]])
            n_head += 1
    ms, with_flag, without = [], [], []
    with decode._attached(api, decode._open_decoder(api, sq, fa, 0, "gpu"), sq, bed_path, 0) as dec:
        for rep in range(REPEATS + 1):
            for flag, wall in ((True, with_flag), (False, without)):
                t0 = time.perf_counter()
                _, n, _ = dec.decode_bam(data, skip=skip, ref_to_sq=ref_to_sq, complete=True, end=True, on_device=True, features=flag)
                if rep:
                    wall.append(time.perf_counter() - t0)
            if rep:
                ms.append(dec.annot_ms())
    return {"records": int(n), "annotation_pass_ms_events": spread(ms), "call_seconds_with_flag": spread(with_flag),
            "call_seconds_without_flag": spread(without),
            "note": "one gs_decode_bam_device call over the whole file, the text copied back to the host inside the timed call; the pass is "
                    "k_dc_feat between two stream events"}


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    out_path = Path(args.get("out", ROOT / "profiles" / "decode_annotate_rate.json"))
    parent = args.get("parent")
    guides = int(args.get("guides", 0))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    say("synthetic chr1-sized genome")
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    lengths = [int(x) for x in lengths]
    bed, _ = make_bed(names[0], lengths[0])
    res = {"workload": "chr1", "genome_bases": lengths[0], "mismatches": M, "mode": "complete", "bgzf": "gpu", "repeats": REPEATS,
           "guides": guides or "all candidates"}
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_dc_annot_", dir=base))
    try:
        raw = np.asarray(text)
        raw.tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        with open(d / "g.fa", "wb") as f:
            f.write(b">" + names[0].encode() + b"\n")
            whole = raw.shape[0] // 60 * 60                # lines of 60 symbols, as FASTA files have them
            lines = np.full((whole // 60, 61), 10, np.uint8)
            lines[:, :60] = raw[:whole].reshape(-1, 60)
            f.write(lines.tobytes())
            if whole < raw.shape[0]:
                f.write(raw[whole:].tobytes() + b"\n")
        (d / "a.bed").write_text(bed)
        source = ["--all-candidates"]
        if guides:
            run([CLI, "kmers", d / "g", "-o", d / "all.csv"])
            with open(d / "all.csv") as f, open(d / "some.csv", "w") as o:
                for i, line in enumerate(f):
                    if i > guides:
                        break
                    o.write(line)
            source = ["-f", d / "some.csv"]
        say("the database")
        s, _ = run([CLI, "enumerate", d / "g", "-m", M, "--mode", "complete", "--format", "bam", "--bgzf", "gpu", "--encoder", "gpu",
                    "-o", d / "db.bam"] + source)
        res["enumerate_wall_s"] = s
        res["database_bytes"] = (d / "db.bam").stat().st_size
        runs = {"plain": [], "annotate": [], "parent": []}
        lines = {}
        kinds = [("plain", CLI, None), ("annotate", CLI, d / "a.bed")] + ([("parent", parent, None)] if parent else [])
        for rep in range(REPEATS + 1):
            say(f"command, round {rep}")
            for kind, binary, b in kinds:
                s, line = run(decode_cmd(binary, d / "db.bam", d / "g.fa", d / f"{kind}.csv", b))
                if rep:        # round 0 warms the page cache and the code objects
                    runs[kind].append(s)
                    lines[kind] = line
        rows = 0
        with open(d / "plain.csv", "rb") as f:
            rows = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 26), b"")) - 1
        cmd = {"off_targets": rows, "plain_seconds": spread(runs["plain"]), "annotate_seconds": spread(runs["annotate"]),
               "plain_csv_bytes": (d / "plain.csv").stat().st_size, "annotate_csv_bytes": (d / "annotate.csv").stat().st_size,
               "annotate_differs_from_plain": differs(runs["annotate"], runs["plain"]),
               "annotated_table_without_its_column_is_the_plain_table": same_without_last_column(d / "annotate.csv", d / "plain.csv"),
               "stage_lines": lines, "files_on": base}
        if parent:
            cmd["parent_seconds"] = spread(runs["parent"])
            cmd["plain_slower_than_every_parent_run"] = min(runs["plain"]) > max(runs["parent"])
            cmd["plain_differs_from_parent"] = differs(runs["plain"], runs["parent"])
            cmd["same_bytes_as_parent"] = subprocess.run(["cmp", "-s", str(d / "plain.csv"), str(d / "parent.csv")]).returncode == 0
        else:
            cmd["parent_seconds"] = "not run"
        res["command"] = cmd
        say("the pass alone")
        res["pass"] = pass_alone(d / "db.bam", d / "g.fa", d / "a.bed")
        res["pass"]["off_targets"] = rows
        res["pass"]["off_targets_per_second_median"] = rows / (1e-3 * res["pass"]["annotation_pass_ms_events"]["median"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())

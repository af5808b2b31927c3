#!/usr/bin/env python3
"""What reading the genome's FASTA costs, on the host and on the device (gs_fasta.hip, `--fasta host|gpu` of `guidescan
index` and `guidescan decode`), recorded in profiles/fasta_rate.json - a record, not a threshold.  The input is a synthetic
FASTA of the genome of synth.py at the given size, 60 symbols per line, on /dev/shm.  Every figure is the median of three
runs after one run that is not counted (it warms the page cache, the device and the library); all values are kept.
  (a) the host readers as the binary given with --parent runs them (the commit before the device reader; without
      --parent this tree's binary with --fasta host, and the file says so): `index` without --store-sa, wall time of the
      command, and `decode`'s "FASTA read" stage on a database of no records (its @SQ lines only);
      and `index --fasta host --verbose` of this tree, whose stage line splits the command into the FASTA read and the
      .gs / .dna writes (the parent's `index` has no such line);
  (b) --fasta gpu of this tree, the same figures with the stage lines of both commands (for `index`: FASTA read, the
      writes, and inside the read the file reads, the waits for the uploads, the device stage, the names, the text copied
      back; "unattributed_s" is the wall clock beyond the two stages: the process's start and end), and the same library
      calls made in this process, where the device is already up;
  (c) the passes alone, timed by events in the stream: milliseconds per pass, GB/s of raw input over their sum, and the
      bytes the passes must move (three reads of the raw file and one write of the text).  The "device stage" of (b) is a
      host clock around the passes, the allocations between them and the waits for their results.
    python tools/fasta_rate.py [--workload hg38] [--parent PATH/TO/guidescan] [--out profiles/fasta_rate.json]"""
import argparse
import json
import os
import re
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
api = import_module("guidescan-cli_amd.api")
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
RUNS = 3
GPU_STAGES = (r"fasta gpu: file reads ([0-9.]+) s, waits for the uploads ([0-9.]+) s, device stage ([0-9.]+) s \(its five passes ([0-9.]+) s\), "
              r"titles and names ([0-9.]+) s")
GPU_KEYS = ("file_reads_s", "upload_waits_s", "device_stage_s", "passes_s", "names_s")


def note(msg):
    print(f"[fasta_rate] {msg}", file=sys.stderr, flush=True)


def write_fasta(path, text, names, lengths, width=60):
    """synth.write_fasta's file, written through numpy (a Python loop over 5x10^7 lines takes minutes)"""
    with open(path, "wb") as f:
        off = 0
        for nm, ln in zip(names, lengths):
            f.write(b">" + nm.encode() + b" synthetic\n")
            full = ln // width
            block = np.empty((full, width + 1), dtype=np.uint8)
            block[:, :width] = text[off:off + full * width].reshape(full, width)
            block[:, width] = 10
            block.tofile(f)
            if ln % width:
                f.write(text[off + full * width:off + ln].tobytes() + b"\n")
            off += ln


def timed(cmd, timeout=1500):
    t0 = time.perf_counter()
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"{cmd[:3]}: {r.stderr[-400:]}")
    return wall, r.stderr


def repeat(fn):
    fn()   # not counted
    vals = [fn() for _ in range(RUNS)]
    return vals


def med(dicts):
    """median per key of a list of flat dicts"""
    return {k: statistics.median(d[k] for d in dicts) for k in dicts[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="hg38")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fasta_rate.json"))
    a = ap.parse_args()
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[a.workload]
    note("genome")
    text, names, lengths = synth.make_genome(lengths, seed=1)
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_fa_", dir=base))
    res = {"workload": a.workload, "files_on": base, "runs": RUNS, "line_width": 60}
    try:
        fa = d / "g.fa"
        write_fasta(fa, np.asarray(text), names, lengths)
        text_len = int(np.asarray(text).shape[0])
        del text
        raw_bytes = fa.stat().st_size
        res.update(fasta_bytes=raw_bytes, text_bytes=text_len, records=len(names))
        (d / "empty.sam").write_text("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in zip(names, lengths)))
        host_cli = Path(a.parent) if a.parent else CLI
        host_flags = [] if a.parent else ["--fasta", "host"]
        res["host_reader_binary"] = "the parent commit's" if a.parent else "this tree's, --fasta host"

        def index_wall(cli, flags, prefix):
            wall, err = timed([cli, "index", "--index", d / prefix] + flags + [fa])
            out = {"wall_s": wall}
            m = re.search(r"Stages: FASTA read ([0-9.]+) s, \.gs and \.dna writes ([0-9.]+) s", err)
            if m:
                out.update(fasta_read_s=float(m.group(1)), writes_s=float(m.group(2)))
                out["unattributed_s"] = wall - out["fasta_read_s"] - out["writes_s"]
            m = re.search(GPU_STAGES + r", text back ([0-9.]+) s", err)
            if m:
                out.update(zip(GPU_KEYS + ("text_back_s",), map(float, m.groups())))
            return out

        def decode_stage(cli, flags):
            wall, err = timed([cli, "decode", "--verbose"] + flags + ["-o", d / "out.csv", d / "empty.sam", fa])
            m = re.search(r"FASTA read ([0-9.]+) s", err)
            out = {"wall_s": wall, "fasta_read_s": float(m.group(1))}
            m = re.search(GPU_STAGES, err)
            if m:
                out.update(zip(GPU_KEYS, map(float, m.groups())))
                out["unattributed_s"] = out["fasta_read_s"] - out["file_reads_s"] - out["upload_waits_s"] - out["device_stage_s"] - out["names_s"]
            return out

        note("(a) host readers")
        v = repeat(lambda: index_wall(host_cli, host_flags, "host"))
        res["a_index_host"] = {"runs": v, "median": med(v)}
        v = repeat(lambda: decode_stage(host_cli, host_flags))
        res["a_decode_host"] = {"runs": v, "median": med(v)}
        v = repeat(lambda: index_wall(CLI, ["--fasta", "host", "--verbose"], "host2"))
        res["a_index_host_this_tree"] = {"runs": v, "median": med(v)}
        (d / "host2.dna").unlink()
        note("(b) --fasta gpu")
        v = repeat(lambda: index_wall(CLI, ["--fasta", "gpu", "--verbose"], "gpu"))
        res["b_index_gpu"] = {"runs": v, "median": med(v)}
        res["b_index_files_equal"] = all((d / f"gpu.{e}").read_bytes() == (d / f"host.{e}").read_bytes() for e in ("gs",)) and \
            subprocess.run(["cmp", "-s", str(d / "gpu.dna"), str(d / "host.dna")]).returncode == 0
        v = repeat(lambda: decode_stage(CLI, ["--fasta", "gpu"]))
        res["b_decode_gpu"] = {"runs": v, "median": med(v)}

        def library(rules):
            t0 = time.perf_counter()
            f = api.DeviceFasta.parse(fa, rules)
            t_parse = time.perf_counter() - t0
            ms = f.ms()
            out = {"parse_call_s": t_parse, "file_reads_s": ms["read"] / 1e3, "upload_waits_s": ms["upload"] / 1e3,
                   "device_stage_s": ms["kernels"] / 1e3, "passes_s": sum(ms["passes"].values()) / 1e3, "names_s": ms["names"] / 1e3}
            out.update({f"pass_{k}_ms": x for k, x in ms["passes"].items()})
            if rules == "index":
                p = api.C.c_void_p()
                t0 = time.perf_counter()
                api._check(api.lib().gs_fasta_text(f._h, 0, api.C.byref(p)))
                out["text_back_s"] = time.perf_counter() - t0
            f.close()
            return out

        note("(b, c) the library calls")
        for rules in ("index", "records"):
            v = repeat(lambda: library(rules))
            m = med(v)
            res[f"b_library_{rules}"] = {"runs": v, "median": m}
            res[f"c_kernels_{rules}"] = {
                "passes_sum_ms": m["passes_s"] * 1e3, "device_stage_ms": m["device_stage_s"] * 1e3, "raw_GB_per_s": raw_bytes / m["passes_s"] / 1e9,
                "bytes_moved_at_least": 3 * raw_bytes + text_len, "moved_GB_per_s": (3 * raw_bytes + text_len) / m["passes_s"] / 1e9,
                "passes_ms": {k[5:-3]: m[k] for k in m if k.startswith("pass_")},
                "longest_pass": max((k[5:-3] for k in m if k.startswith("pass_")), key=lambda k: m[f"pass_{k}_ms"])}
        res["index_gpu_over_host"] = res["b_index_gpu"]["median"]["wall_s"] / res["a_index_host"]["median"]["wall_s"]
        res["decode_fasta_read_gpu_over_host"] = res["b_decode_gpu"]["median"]["fasta_read_s"] / res["a_decode_host"]["median"]["fasta_read_s"]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if not k.startswith(("a_", "b_"))}, indent=1))


if __name__ == "__main__":
    main()

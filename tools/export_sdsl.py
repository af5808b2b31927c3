#!/usr/bin/env python3
"""Time GenomeIndex.save_sdsl (the reference's index files from the GPU-built index, gs_sdsl_export.hip) on a synthetic
genome, twice (the first call carries code loading), and - where oracle/_ref is built - the compiled reference
containers' writer from the same suffix arrays (two host threads, one per strand); compare the files byte for byte, on a
difference name the first section of the SURVEY.md App. A walk that differs.  Prints progress lines and, last, one JSON
line.
Usage (GPU box, repo root): python tools/export_sdsl.py [workload=hg38] [--dir DIR]"""
import json
import os
import shutil
import sys
import tempfile
import threading
import time
from importlib import import_module
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def first_difference(a, b, chunk=1 << 26):
    """offset of the first differing byte of two files, or None"""
    at = 0
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(chunk), fb.read(chunk)
            if x != y:
                m = min(len(x), len(y))
                return at + next((i for i in range(m) if x[i] != y[i]), m)
            if not x:
                return None
            at += len(x)


def main():
    import numpy as np
    import torch
    torch.zeros(1, device="cuda")
    bench = import_module("bench")
    api = import_module("guidescan-cli_amd.api")
    synth = import_module("guidescan-cli_amd.synth")
    import oracle_lib as ol
    from sdsl_walk import walk

    args = sys.argv[1:]
    where = None
    if "--dir" in args:
        i = args.index("--dir")
        where = args[i + 1]
        del args[i:i + 2]
    workload = args[0] if args else "hg38"
    lens_name, batch, probs = bench.WORKLOADS[workload]
    lengths = [synth.CHR1_LENGTH] if lens_name == "CHR1" else getattr(synth, lens_name)
    text, names, lengths = bench.make_workload_genome(synth, workload, lengths, probs)
    n = text.shape[0] + 1
    print(f"{workload}: {text.shape[0]} symbols", flush=True)
    if where is None:
        where = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 3 * n else tempfile.gettempdir()
    d = tempfile.mkdtemp(prefix="gs_export_", dir=where)
    out = dict(workload=workload, symbols=int(text.shape[0]), files_in=where)
    try:
        t0 = time.time()
        g = api.GenomeIndex.build(text, device=0)
        out["build_s"] = round(time.time() - t0, 2)
        print(f"index built in {out['build_s']} s", flush=True)
        times = []
        for k in range(2):
            t0 = time.time()
            g.save_sdsl(text, os.path.join(d, "ours"))
            times.append(round(time.time() - t0, 2))
            print(f"save_sdsl call {k + 1}: {times[-1]} s", flush=True)
        out["save_sdsl_s"] = times
        out["scratch_peak_bytes"] = api.sdsl_export_scratch()
        out["scratch_bytes_per_base"] = round(out["scratch_peak_bytes"] / text.shape[0], 3)
        out["bytes"] = [os.path.getsize(os.path.join(d, "ours" + s)) for s in (".forward", ".reverse")]
        ref = ol.ref()
        if ref is not None:
            err = []

            def one(strand, suffix):
                try:
                    sa = g.suffix_array(strand)
                    st = np.ascontiguousarray(text if strand == 0 else synth.reverse_complement_bytes(text))
                    h = ref.ref_index_build_text(st.ctypes.data, sa.ctypes.data, n, os.path.join(d, f"tmp{strand}.sdsl").encode())
                    assert ref.ref_write_index_file(h, os.path.join(d, "ref" + suffix).encode()) == 0
                    ref.ref_index_free(h)
                except Exception as e:
                    err.append(repr(e))

            t0 = time.time()
            th = [threading.Thread(target=one, args=a) for a in ((0, ".forward"), (1, ".reverse"))]
            for t in th:
                t.start()
            while any(t.is_alive() for t in th):
                th[0].join(60)
                print(f"reference writer: {time.time() - t0:.0f} s", flush=True)
            for t in th:
                t.join()
            assert not err, err
            out["reference_writer_s"] = round(time.time() - t0, 2)
            out["reference_bytes"] = [os.path.getsize(os.path.join(d, "ref" + s)) for s in (".forward", ".reverse")]
            same = True
            for s in (".forward", ".reverse"):
                at = first_difference(os.path.join(d, "ours" + s), os.path.join(d, "ref" + s))
                if at is not None:
                    same = False
                    with open(os.path.join(d, "ref" + s), "rb") as f:
                        sec, _ = walk(f.read())
                    out["first_difference" + s] = dict(byte=at, section=[k for k, (a, b) in sec.items() if a <= at < b])
            out["bytes_equal"] = same
            out["export_is_faster"] = max(times) < out["reference_writer_s"]
        g.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out), flush=True)
    return 0 if out.get("bytes_equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())

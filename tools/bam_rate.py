#!/usr/bin/env python3
"""What writing a BAM database on the device (GS_TEXT_BAM records + gs_bgzf.hip) costs and what it saves, on one GPU:
  (a) event-timed milliseconds and GB/s of gs_bgzf_compress_device on one batch's BAM records, five calls after the
      first; beside it the GB/s of 16 host threads running zlib's raw deflate at level 6 over the same 0xff00-byte
      pieces (what bam::bgzf_append does in the CLI's formatting threads), same session;
  (b) the compressed bytes, beside zlib level 6 and level 1 over the same pieces; the condition: not above level 1;
  (c) wall time of the built `guidescan enumerate --format bam`, end to end, --bgzf host against --bgzf gpu: three
      interleaved runs each, every value, the medians, the stage seconds; the condition: gpu median <= host median.
    python tools/bam_rate.py [workload=hg38] [n_guides=1000000] [out=profiles/bam_rate.json]
The genome is bench.py's synthetic one of that size; 1 M NGG 20-mers, m <= 3, complete mode, files in /dev/shm."""
import ctypes as C
import gzip
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
synth = import_module("guidescan-cli_amd.synth")
api = import_module("guidescan-cli_amd.api")

THREADS = 16
PIECE = 0xff00


def deflate_pieces(raw, level, lo, hi):
    """compressed bytes of pieces [lo, hi), each a gzip member as bam::bgzf_append frames it (26 bytes around the stream)"""
    total = 0
    for k in range(lo, hi):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        total += len(z.compress(raw[k * PIECE:(k + 1) * PIECE])) + len(z.flush()) + 26
    return total


def host_deflate(raw, level):
    """-> (seconds, compressed bytes) with THREADS threads, a contiguous range of pieces each (zlib releases the GIL)"""
    n_p = (len(raw) + PIECE - 1) // PIECE
    with ThreadPoolExecutor(THREADS) as ex:
        t0 = time.perf_counter()
        sizes = list(ex.map(lambda t: deflate_pieces(raw, level, n_p * t // THREADS, n_p * (t + 1) // THREADS), range(THREADS)))
        return time.perf_counter() - t0, sum(sizes)


def main():
    import torch
    workload = sys.argv[1] if len(sys.argv) > 1 else "hg38"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "bam_rate.json"
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[workload]
    torch.zeros(1, device="cuda")
    text, names, lengths = synth.make_genome(lengths, seed=1)
    seqs, pams, pos, strands = synth.sample_guides(text, n, seed=7777)
    gs = api.make_genome_structure(names, lengths)
    ids = [f"g{i}" for i in range(n)]
    senses = [chr(s) == "+" for s in strands]
    res = {"workload": workload, "guides": n, "mismatches": 3, "format": "bam complete"}

    def save():
        out_path.write_text(json.dumps(res, indent=1) + "\n")

    # the CLI's files first: the in-process index then has the card to itself
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_bam_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        sq = [x.decode() for x in np.ascontiguousarray(seqs).view(f"S{seqs.shape[1]}").ravel()]
        (d / "k.csv").write_text("id,sequence,pam,chromosome,position,sense\n" +
                                 "".join(f"g{i},{sq[i]},NGG,chr1,{int(pos[i]) + 1},{chr(strands[i])}\n" for i in range(n)))
        cli = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
        env = dict(os.environ)
        env.pop("GS_ENCODER", None)
        c, inflated = {}, {}
        for mode in ("host", "gpu", "host", "gpu", "host", "gpu"):  # interleaved: a drifting box moves both alike
            o = d / f"o.{mode}.bam"
            if o.exists():
                o.unlink()
            t0 = time.perf_counter()
            r = subprocess.run([str(cli), "enumerate", str(d / "g"), "-f", str(d / "k.csv"), "-o", str(o), "-m", "3", "--format", "bam",
                                "--bgzf", mode, "-n", str(THREADS)], capture_output=True, text=True, timeout=900, env=env)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-400:])
            e = c.setdefault(mode, {"seconds_after_index_load": [], "wall_s": [], "stages": [], "bytes": 0})
            e["seconds_after_index_load"].append(float(re.search(r"Processed \d+ kmers in ([0-9.eE+-]+) seconds", r.stdout).group(1)))
            e["wall_s"].append(wall)
            m = re.search(r"device ([0-9.eE+-]+) s, text formatting ([0-9.eE+-]+) s, file writes ([0-9.eE+-]+) s", r.stdout)
            e["stages"].append({"device": float(m.group(1)), "text_formatting": float(m.group(2)), "file_writes": float(m.group(3))})
            e["bytes"] = o.stat().st_size
            m = re.search(r"encoder: bgzf gpu \((\d+) batch\(es\) compressed on the device, (\d+)", r.stdout)
            if m:
                e["batches_device_host"] = [int(m.group(1)), int(m.group(2))]
        for mode in ("host", "gpu"):
            with gzip.open(d / f"o.{mode}.bam", "rb") as fh:
                import hashlib
                h = hashlib.sha256()
                for blk in iter(lambda: fh.read(1 << 24), b""):
                    h.update(blk)
                inflated[mode] = h.hexdigest()
        for e in c.values():
            e["median_seconds_after_index_load"] = statistics.median(e["seconds_after_index_load"])
            e["median_wall_s"] = statistics.median(e["wall_s"])
        c["same_records"] = inflated["host"] == inflated["gpu"]
        c["gpu_median_not_above_host_median"] = c["gpu"]["median_seconds_after_index_load"] <= c["host"]["median_seconds_after_index_load"]
        c["output_on"] = base
        res["c_cli_end_to_end"] = c
        save()
    finally:
        shutil.rmtree(d, ignore_errors=True)

    gidx = api.GenomeIndex.build(text, device=0)
    try:
        L, P = seqs.shape[1], pams.shape[1]
        d_s, d_p = torch.from_numpy(seqs).cuda(), torch.from_numpy(pams).cuda()
        d_spec = torch.empty(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        with gidx.locked():
            d_off, d_hits, st = gidx.enumerate_device(d_s.data_ptr(), n, L, d_p.data_ptr(), P, mismatches=3)
            gidx.score_device(gs, d_s.data_ptr(), n, L, P, d_off, d_hits, None, d_spec.data_ptr(), sam=True)
            ms_rec = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                d_rec, ln = gidx.format_device(gs, d_s.data_ptr(), n, L, d_p.data_ptr(), P, ids, senses, None, d_off, d_hits,
                                               d_spec.data_ptr(), 3, bam=True, complete=True)
                e1.record()
                torch.cuda.synchronize()
                ms_rec.append(e0.elapsed_time(e1))
            ms, out_len = [], 0
            for _ in range(6):  # the first call sizes the handle's buffers
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                d_out, out_len = gidx.bgzf_compress_device(d_rec, ln)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            raw = np.empty(ln, np.uint8)
            assert hip.hipMemcpy(raw.ctypes.data, d_rec, ln, 2) == 0
            members = np.empty(out_len, np.uint8)
            assert hip.hipMemcpy(members.ctypes.data, d_out, out_len, 2) == 0
        raw = raw.tobytes()
        round_trip = gzip.decompress(members.tobytes()) == raw
        med = statistics.median(ms[1:])
        res["a_device_compress"] = {"record_bytes": ln, "hits": st["n_hits"], "ms_records_each_call_incl_upload_of_ids": ms_rec,
                                    "ms_each_call": ms, "ms_median_after_first": med, "ms_min_after_first": min(ms[1:]),
                                    "GB_per_s_median": ln / (med * 1e-3) / 1e9, "inflates_to_the_records": round_trip}
        save()
        t6 = [host_deflate(raw, 6) for _ in range(2)]
        t1 = host_deflate(raw, 1)
        res["a_host_zlib"] = {"threads": THREADS, "level6_seconds_each": [t[0] for t in t6],
                              "level6_GB_per_s": ln / min(t[0] for t in t6) / 1e9, "level1_seconds": t1[0],
                              "level1_GB_per_s": ln / t1[0] / 1e9}
        res["b_size"] = {"device_bytes": out_len, "zlib_level6_bytes": t6[0][1], "zlib_level1_bytes": t1[1],
                         "device_over_raw": out_len / ln, "level6_over_raw": t6[0][1] / ln, "level1_over_raw": t1[1] / ln,
                         "device_not_above_level1": out_len <= t1[1]}
    finally:
        gidx.close()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

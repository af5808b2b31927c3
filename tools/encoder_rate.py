#!/usr/bin/env python3
"""What the device text encoder (gs_textdev.hip) costs and what it saves, on one GPU:
  (a) event-timed milliseconds of gs_format_device on one batch, its bytes, and the floor its traffic sets
      (text bytes written + 16 B per hit read, at the HBM rate a streaming kernel reaches on an MI355X);
  (b) seconds of gs_format_guides_scored - the host encoder - on the same batch, 16 threads, a guide range each
      (what the CLI's formatting threads do);
  (c) wall time of the built `guidescan enumerate`, end to end, with --encoder host and --encoder gpu: three runs each,
      the median and every value.
    python tools/encoder_rate.py [workload=hg38] [n_guides=1000000] [out=profiles/encoder_rate.json]
The genome is bench.py's synthetic one of that size; 1 M NGG 20-mers, m <= 3, CSV complete."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
synth = import_module("guidescan-cli_amd.synth")
api = import_module("guidescan-cli_amd.api")

HBM_ACHIEVABLE_GBS = 6300.0  # what a streaming copy reaches on an MI355X (8 TB/s peak)
THREADS = 16


def main():
    import torch
    workload = sys.argv[1] if len(sys.argv) > 1 else "hg38"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "encoder_rate.json"
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[workload]
    torch.zeros(1, device="cuda")
    text, names, lengths = synth.make_genome(lengths, seed=1)
    seqs, pams, pos, strands = synth.sample_guides(text, n, seed=7777)
    gs = api.make_genome_structure(names, lengths)
    ids = [f"g{i}" for i in range(n)]
    senses = [chr(s) == "+" for s in strands]
    res = {"workload": workload, "guides": n, "mismatches": 3, "format": "csv complete"}

    # the CLI's files first: the in-process index then has the card to itself
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_enc_", dir=base))
    try:
        np.asarray(text).tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        sq = [x.decode() for x in np.ascontiguousarray(seqs).view(f"S{seqs.shape[1]}").ravel()]
        (d / "k.csv").write_text("id,sequence,pam,chromosome,position,sense\n" +
                                 "".join(f"g{i},{sq[i]},NGG,chr1,{int(pos[i]) + 1},{chr(strands[i])}\n" for i in range(n)))
        cli = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
        env = dict(os.environ)
        env.pop("GS_ENCODER", None)
        c = {}
        for enc in ("host", "gpu", "host", "gpu", "host", "gpu"):  # interleaved: a drifting box moves both alike
            o = d / "o.csv"
            if o.exists():
                o.unlink()
            t0 = time.perf_counter()
            r = subprocess.run([str(cli), "enumerate", str(d / "g"), "-f", str(d / "k.csv"), "-o", str(o), "-m", "3", "--encoder", enc,
                                "-n", str(THREADS)], capture_output=True, text=True, timeout=900, env=env)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-400:])
            e = c.setdefault(enc, {"seconds_after_index_load": [], "wall_s": [], "stages": [], "sha256": set(), "bytes": 0})
            e["seconds_after_index_load"].append(float(re.search(r"Processed \d+ kmers in ([0-9.eE+-]+) seconds", r.stdout).group(1)))
            e["wall_s"].append(wall)
            m = re.search(r"device ([0-9.eE+-]+) s, text formatting ([0-9.eE+-]+) s, file writes ([0-9.eE+-]+) s", r.stdout)
            e["stages"].append({"device": float(m.group(1)), "text_formatting": float(m.group(2)), "file_writes": float(m.group(3))})
            h = hashlib.sha256()
            with open(o, "rb") as fh:
                for blk in iter(lambda: fh.read(1 << 24), b""):
                    h.update(blk)
            e["sha256"].add(h.hexdigest())
            e["bytes"] = o.stat().st_size
        for e in c.values():
            e["median_seconds_after_index_load"] = statistics.median(e["seconds_after_index_load"])
            e["median_wall_s"] = statistics.median(e["wall_s"])
            e["sha256"] = sorted(e["sha256"])
        c["files_identical"] = c["host"]["sha256"] == c["gpu"]["sha256"] and len(c["host"]["sha256"]) == 1
        c["gpu_median_not_above_host_median"] = c["gpu"]["median_seconds_after_index_load"] <= c["host"]["median_seconds_after_index_load"]
        c["output_on"] = base
        res["c_cli_end_to_end"] = c
    finally:
        shutil.rmtree(d, ignore_errors=True)

    gidx = api.GenomeIndex.build(text, device=0)
    try:
        L, P = seqs.shape[1], pams.shape[1]
        d_s, d_p = torch.from_numpy(seqs).cuda(), torch.from_numpy(pams).cuda()
        d_spec = torch.empty(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with gidx.locked():
            d_off, d_hits, st = gidx.enumerate_device(d_s.data_ptr(), n, L, d_p.data_ptr(), P, mismatches=3)
            gidx.score_device(gs, d_s.data_ptr(), n, L, P, d_off, d_hits, None, d_spec.data_ptr())
            # the C entry itself between the events: the id blob and the sense bytes are made once, ahead of the calls
            blob, id_off = api._id_blob(ids)
            keep = C.create_string_buffer(blob, len(blob) + 1)
            se = np.asarray(senses, np.uint8)
            d_text, tl = C.c_void_p(), C.c_uint64()
            ms, wall_ms = [], []
            for _ in range(5):  # the first call sizes the handle's buffers
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                rc = api.lib().gs_format_device(gidx._h, C.byref(gs), d_s.data_ptr(), n, L, d_p.data_ptr(), P, C.addressof(keep),
                                                id_off.ctypes.data, se.ctypes.data, None, d_off, d_hits, d_spec.data_ptr(), 3,
                                                api.GS_TEXT_COMPLETE, -1, None, C.byref(d_text), C.byref(tl))
                e1.record()
                torch.cuda.synchronize()
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
                ms.append(e0.elapsed_time(e1))
            d_text, ln = d_text.value, int(tl.value)
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            dev_text = np.empty(ln, np.uint8)
            assert hip.hipMemcpy(dev_text.ctypes.data, d_text, ln, 2) == 0
            offsets = np.empty(n + 1, np.uint64)
            hits = np.empty(st["n_hits"], api.HIT_DTYPE)
            assert hip.hipMemcpy(offsets.ctypes.data, d_off, 8 * (n + 1), 2) == 0
            assert hip.hipMemcpy(hits.ctypes.data, d_hits, 16 * st["n_hits"], 2) == 0
        spec = d_spec.cpu().numpy()
        traffic = ln + 16 * st["n_hits"]
        res["a_device_encode"] = {"ms_each_call_incl_upload_of_ids": ms, "ms_min_after_first": min(ms[1:]),
                                  "host_wall_ms_each_call": wall_ms, "text_bytes": ln, "hits": st["n_hits"],
                                  "GB_per_s_text": ln / (min(ms[1:]) * 1e-3) / 1e9,
                                  "floor_ms_from_traffic": traffic / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3,
                                  "floor_assumes_GB_per_s": HBM_ACHIEVABLE_GBS, "traffic_bytes": traffic}
        # (b) the host encoder, 16 threads, a contiguous guide range each (ctypes releases the GIL)
        sq = [x.decode() for x in np.ascontiguousarray(seqs).view(f"S{L}").ravel()]
        kmers = (api.GsKmer * n)(*[api.GsKmer(ids[i].encode(), sq[i].encode(), b"NGG", int(senses[i])) for i in range(n)])
        Lb = api.lib()

        def part(t):
            lo, hi = n * t // THREADS, n * (t + 1) // THREADS
            out, k = C.c_void_p(), C.c_size_t()
            rc = Lb.gs_format_guides_scored(C.byref(gs), C.byref(kmers, lo * C.sizeof(api.GsKmer)), hi - lo, offsets[lo:].ctypes.data,
                                            hits.ctypes.data, spec[lo:].ctypes.data, None, 3, api.GS_TEXT_COMPLETE, -1, C.byref(out),
                                            C.byref(k))
            assert rc == 0
            return out, k.value

        secs, same = [], None
        for rep in range(3):
            with ThreadPoolExecutor(THREADS) as ex:
                t0 = time.perf_counter()
                parts = list(ex.map(part, range(THREADS)))
                secs.append(time.perf_counter() - t0)
            if rep == 0:
                host_text = b"".join(C.string_at(p, k) for p, k in parts)
                same = host_text == dev_text.tobytes()
                del host_text
            for p, _ in parts:
                Lb.gs_free(p)
        res["b_host_encode"] = {"threads": THREADS, "seconds_each": secs, "seconds_min": min(secs), "same_bytes_as_device": same}
    finally:
        gidx.close()
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

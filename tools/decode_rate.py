#!/usr/bin/env python3
"""What decoding an off-target database costs on one GPU (gs_decode.hip, `guidescan decode`), recorded in
profiles/decode_rate.json - a record, not a threshold:
  (a) wall time of the built `guidescan decode --mode complete`, end to end (FASTA and SAM read, decode, CSV written):
      three runs, the median and every value, off-targets/s and output GB/s;
  (b) the device stage alone: gs_decode_records_device on the whole database as one batch whose arrays are made ahead
      of the calls - the upload of the batch, the kernels and the scans, the text left in HBM; a host clock around the
      call, which ends in a device synchronise; the first call (it sizes the decoder's buffers) is not counted;
  (c) the Python model (decode.py) on the first 10,000 records, on the same box;
  (d) the same database written with `--format bam`, through `guidescan decode --bgzf host` and `--bgzf gpu`: three runs
      each, taking turns, the medians, the stage lines, the two tables compared byte for byte; the one condition is that of
      bam_rate.json: the --bgzf gpu median does not exceed the --bgzf host median on the same box;
  (e) the device stages of the BAM route alone: gs_decode_bam_device on the whole file as one call, five calls after the
      first, split into inflate (with the upload of the compressed bytes), record starts, fields and the decoder's kernels
      (host clocks around stages that end in a device synchronise);
  (f) inflate in GB/s of output, beside host zlib on 16 threads over the same members.
    python tools/decode_rate.py [workload=hg38] [n_guides=1000000] [out=profiles/decode_rate.json] [sections=abcdef]
Sections left out keep the values the output file already holds.
The database is made here by our own `guidescan enumerate --format sam --mode complete -m 3` over bench.py's synthetic
genome of that size and NGG 20-mers sampled from it.  The reference script itself (pysam, Biopython) cannot run here."""
import ctypes as C
import json
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
synth = import_module("guidescan-cli_amd.synth")
api = import_module("guidescan-cli_amd.api")
decode = import_module("guidescan-cli_amd.decode")
CLI = ROOT / "guidescan-cli_amd" / "bin" / "guidescan"


STAGES = []  # the last stderr line of every command run


def note(msg):
    print(f"[decode_rate] {msg}", file=sys.stderr, flush=True)


def run(cmd, timeout):
    note(" ".join(str(c) for c in cmd[:2]))
    t0 = time.perf_counter()
    r = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError(f"{cmd[1]}: {r.stderr[-400:]}")
    STAGES.append(r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "")
    return time.perf_counter() - t0


def main():
    workload = sys.argv[1] if len(sys.argv) > 1 else "hg38"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    out_path = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "decode_rate.json"
    sections = sys.argv[4] if len(sys.argv) > 4 else "abcdef"
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[workload]
    note("genome")
    text, names, lengths = synth.make_genome(lengths, seed=1)
    seqs, pams, pos, strands = synth.sample_guides(text, n, seed=7777)
    res = {"workload": workload, "guides": n, "mismatches": 3, "mode": "complete"}
    if out_path.exists() and set(sections) != set("abcdef"):
        old = json.loads(out_path.read_text())
        if (old.get("workload"), old.get("guides")) == (workload, n):
            res = old
    base = os.environ.get("GS_E2E_DIR") or ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp")
    d = Path(tempfile.mkdtemp(prefix="gs_dec_", dir=base))
    try:
        text = np.asarray(text)
        text.tofile(d / "g.dna")
        (d / "g.gs").write_text("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        with open(d / "g.fa", "wb") as f:  # one line per record
            at = 0
            for name, ln in zip(names, lengths):
                f.write(f">{name}\n".encode())
                f.write(text[at:at + ln].tobytes())
                f.write(b"\n")
                at += ln
        sq = [x.decode() for x in np.ascontiguousarray(seqs).view(f"S{seqs.shape[1]}").ravel()]
        (d / "k.csv").write_text("id,sequence,pam,chromosome,position,sense\n" +
                                 "".join(f"g{i},{sq[i]},NGG,chr1,{int(pos[i]) + 1},{chr(strands[i])}\n" for i in range(n)))
        if set("abc") & set(sections):
            res["enumerate_wall_s"] = run([CLI, "enumerate", d / "g", "-f", d / "k.csv", "-o", d / "db.sam", "-m", "3", "--format", "sam",
                                           "--mode", "complete", "--encoder", "gpu", "-n", "16"], 1500)
            res["database_bytes"] = (d / "db.sam").stat().st_size
        if set("def") & set(sections):
            res["bam_enumerate_wall_s"] = run([CLI, "enumerate", d / "g", "-f", d / "k.csv", "-o", d / "db.bam", "-m", "3", "--format", "bam",
                                               "--mode", "complete", "--bgzf", "gpu", "-n", "16"], 1500)
            res["bam_database_bytes"] = (d / "db.bam").stat().st_size

        fasta = {name: text[a:a + ln].tobytes().decode() for name, a, ln in zip(names, np.cumsum([0] + list(lengths[:-1])), lengths)}
        if set("def") & set(sections):
            bam_sections(d, res, sections, fasta)
        if not set("abc") & set(sections):
            return finish(res, out_path)
        # (a) the command, end to end
        del STAGES[:]
        walls = [run([CLI, "decode", "--mode", "complete", "--verbose", "-o", d / "out.csv", d / "db.sam", d / "g.fa"], 1500) for _ in range(3)]
        out_bytes = (d / "out.csv").stat().st_size
        with open(d / "out.csv", "rb") as f:
            rows = sum(blk.count(b"\n") for blk in iter(lambda: f.read(1 << 24), b"")) - 1
        med = statistics.median(walls)
        res["a_cli_end_to_end"] = {"wall_s": walls, "median_wall_s": med, "off_targets": rows, "output_bytes": out_bytes,
                                   "off_targets_per_s": rows / med, "output_GB_per_s": out_bytes / med / 1e9, "files_on": base,
                                   "stage_lines": list(STAGES)}

        note(f"decode: {walls} s, {rows} off-targets")
        # (b) the device stage alone, (c) the model
        sam = (d / "db.sam").read_text()
        sq_list, records = decode.parse_sam(sam)
        del sam
        note(f"{len(records)} records parsed")
        with api.Decoder(sq_list, fasta, device=0) as dec:
            b, keep = dec._batch(records)
            out, ln, nrows = C.c_void_p(), C.c_uint64(), C.c_uint64()
            secs = []
            for _ in range(6):
                t0 = time.perf_counter()
                api._check(api.lib().gs_decode_records_device(dec._h, C.byref(b), api.GS_TEXT_COMPLETE, 0, C.byref(out), C.byref(ln), C.byref(nrows)))
                secs.append(time.perf_counter() - t0)
            assert nrows.value == rows and ln.value + len(decode.COMPLETE_HEADER) + 1 == out_bytes
            med = statistics.median(secs[1:])
            res["b_device_stage"] = {"records": len(records), "seconds": secs[1:], "first_call_s": secs[0], "median_s": med,
                                     "off_targets_per_s": rows / med, "output_GB_per_s": ln.value / med / 1e9,
                                     "includes": "upload of the batch, kernels and scans; the text stays in HBM"}
        note(f"device stage: {secs}")
        sample = records[:10_000]
        t0 = time.perf_counter()
        model_rows = decode.Decoder(sq_list, fasta).rows(sample, complete=True)
        dt = time.perf_counter() - t0
        res["c_python_model"] = {"records": len(sample), "off_targets": len(model_rows), "seconds": dt,
                                 "off_targets_per_s": len(model_rows) / dt}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    finish(res, out_path)


def finish(res, out_path):
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


def bam_sections(d, res, sections, fasta):
    """(d), (e), (f) over d/db.bam and d/g.fa"""
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    bam, fa = d / "db.bam", d / "g.fa"
    if "d" in sections:
        e2e = {route: {"wall_s": [], "stage_lines": []} for route in ("host", "gpu")}
        for _ in range(3):   # the two routes take turns, so that what else the box does meets both
            for route in ("host", "gpu"):
                del STAGES[:]
                e2e[route]["wall_s"].append(run([CLI, "decode", "--mode", "complete", "--verbose", "--bgzf", route, "-o",
                                                 d / f"out.{route}.csv", bam, fa], 1500))
                e2e[route]["stage_lines"] += STAGES
        for route in ("host", "gpu"):
            e2e[route]["median_wall_s"] = statistics.median(e2e[route]["wall_s"])
            note(f"decode --bgzf {route}: {e2e[route]['wall_s']} s")
        same = subprocess.run(["cmp", "-s", str(d / "out.host.csv"), str(d / "out.gpu.csv")]).returncode == 0
        e2e["tables_equal"] = same
        e2e["output_bytes"] = (d / "out.gpu.csv").stat().st_size
        e2e["gpu_median_not_above_host_median"] = e2e["gpu"]["median_wall_s"] <= e2e["host"]["median_wall_s"]
        res["d_bam_cli_end_to_end"] = e2e
        for route in ("host", "gpu"):
            (d / f"out.{route}.csv").unlink()
    if not set("ef") & set(sections):
        return
    data = bam.read_bytes()
    sizes = decode.bgzf_member_sizes(data)
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    head = b""
    for k in range(len(sizes)):   # the members that hold the header
        head += zlib.decompress(data[offs[k]:offs[k + 1]], 31)
        try:
            sq_list, ref_to_sq, skip = decode.bam_header(head)
            break
        except Exception:
            continue
    with api.Decoder(sq_list, fasta, device=0) as dec:
        calls = []
        for _ in range(6):
            t0 = time.perf_counter()
            text, n, tail = dec.decode_bam(data, skip=skip, ref_to_sq=ref_to_sq, complete=True, end=True, on_device=True)
            wall = time.perf_counter() - t0   # (includes the copy of the text to the host that on_device makes for the caller)
            counts, ms = dec.decode_bam_last()
            calls.append({"ms": ms, "wall_s": wall})
            del text
        later = calls[1:]
        med = {k: statistics.median(c["ms"][k] for c in later) for k in ("inflate", "starts", "fields", "decode")}
        res["e_bam_device_stages"] = {"members": counts["members"], "compressed_bytes": counts["compressed"],
                                      "inflated_bytes": counts["inflated"], "records": counts["records"],
                                      "first_call_ms": calls[0]["ms"], "calls_ms": [c["ms"] for c in later], "median_ms": med,
                                      "starts_cost_more_than_inflate_and_fields": med["starts"] > med["inflate"] + med["fields"],
                                      "includes": "inflate: the upload of the compressed bytes, the member table and the kernel"}
        note(f"device stages: {med}")
        if "f" in sections:
            pieces = [data[offs[k]:offs[min(k + 64, len(sizes))]] for k in range(0, len(sizes), 64)]

            def inflate_piece(p):
                n = 0
                while p:
                    z = zlib.decompressobj(31)
                    n += len(z.decompress(p))
                    p = z.unused_data
                return n
            secs = []
            for _ in range(3):
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as pool:
                    total = sum(pool.map(inflate_piece, pieces))
                secs.append(time.perf_counter() - t0)
            assert total == counts["inflated"]
            res["f_inflate_rate"] = {"device_GB_per_s_of_output": counts["inflated"] / (med["inflate"] * 1e-3) / 1e9,
                                     "device_includes": "the upload of the compressed bytes over the link",
                                     "host_zlib_16_threads_s": secs,
                                     "host_zlib_16_threads_GB_per_s_of_output": counts["inflated"] / statistics.median(secs) / 1e9}
            note(f"inflate: {res['f_inflate_rate']}")


if __name__ == "__main__":
    main()

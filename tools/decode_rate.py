#!/usr/bin/env python3
"""What decoding an off-target database costs on one GPU (gs_decode.hip, `guidescan decode`), recorded in
profiles/decode_rate.json - a record, not a threshold:
  (a) wall time of the built `guidescan decode --mode complete`, end to end (FASTA and SAM read, decode, CSV written):
      three runs, the median and every value, off-targets/s and output GB/s;
  (b) the device stage alone: gs_decode_records_device on the whole database as one batch whose arrays are made ahead
      of the calls - the upload of the batch, the kernels and the scans, the text left in HBM; a host clock around the
      call, which ends in a device synchronise; the first call (it sizes the decoder's buffers) is not counted;
  (c) the Python model (decode.py) on the first 10,000 records, on the same box.
    python tools/decode_rate.py [workload=hg38] [n_guides=1000000] [out=profiles/decode_rate.json]
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
    lengths = {"chr1": [synth.CHR1_LENGTH], "hg38": synth.GRCH38_LENGTHS, "saccer3": synth.SACCER3_LENGTHS}[workload]
    note("genome")
    text, names, lengths = synth.make_genome(lengths, seed=1)
    seqs, pams, pos, strands = synth.sample_guides(text, n, seed=7777)
    res = {"workload": workload, "guides": n, "mismatches": 3, "mode": "complete"}
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
        res["enumerate_wall_s"] = run([CLI, "enumerate", d / "g", "-f", d / "k.csv", "-o", d / "db.sam", "-m", "3", "--format", "sam",
                                       "--mode", "complete", "--encoder", "gpu", "-n", "16"], 1500)
        res["database_bytes"] = (d / "db.sam").stat().st_size

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
        fasta = {name: text[a:a + ln].tobytes().decode() for name, a, ln in zip(names, np.cumsum([0] + list(lengths[:-1])), lengths)}
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
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The two forms of the bulge-aware search side by side at hg38 size (the genome of tools/general_bench.py):

  bulges_m1_rna1_dna1   -m 1 --rna-bulges 1 --dna-bulges 1, --guides guides (general_bench's row and guides)
  bulges_m3_rna1_dna1   -m 3 --rna-bulges 1 --dna-bulges 1, --guides3 guides

Each row: the walk (GS_BULGE_FORM=0: k_search_general, which differs from the parent commit's by the guide-list select, in
the same process on the same box), then the seeded form under GS_BULGE_ROWS = 0, 8, 64 and 512 (the m=3 row: the settings
of --rows3, --repeat3 calls each), every call timed after one warm-up; the seeded result must be the walk's byte for byte
(offsets, hits, raw counts), and the words of gs_debug_bulge_last go next to each figure.
Unless --skip-ref the first --ref-guides guides of the m=1 row are also compared line by line with the compiled
reference (oracle/_ref/gs_ref_enumerate on the box's host cores), both forms.  The genome, the guides and the reference's
lines are tools/general_bench.py's (its Hg38 genome, seed 77, ref_lines): the m=1 row is that tool's row of the same name.

Usage (GPU box, repo root): python tools/bulge_bench.py [--guides 4096] [--guides3 256] [--repeat 3] [--out FILE]
Prints one JSON object (and rewrites FILE after every row); profiles/bulge_seeded.json is a run of it."""
import argparse
import json
import os
import sys
import time
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

LAST = ("guides_seeded", "guides_walked", "seeds", "seeds_empty", "row_nodes", "interval_nodes", "exception_lookups",
        "largest_stack")


def timed(gidx, seqs, pams, cfg, repeat):
    gidx.enumerate_general(seqs[:4], pams[:4], **cfg)
    res, secs = None, []
    for _ in range(repeat):
        t0 = time.perf_counter()
        res = gidx.enumerate_general(seqs, pams, raw=True, **cfg)
        secs.append(time.perf_counter() - t0)
    return res, secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guides", type=int, default=4096)
    ap.add_argument("--guides3", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--repeat3", type=int, default=1, help="timed calls per figure of the m=3 row")
    ap.add_argument("--rows3", default="0", help="GS_BULGE_ROWS settings of the m=3 row, comma separated")
    ap.add_argument("--ref-guides", type=int, default=256)
    ap.add_argument("--skip-ref", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    api = import_module("guidescan-cli_amd.api")
    synth = import_module("guidescan-cli_amd.synth")
    full = import_module("test_gpu_fullsize")
    gb = import_module("general_bench")
    h = full.Hg38()
    out = {"genome_bp": int(h.text.shape[0]), "index_build_s": round(h.t_build, 1), "host_threads": os.cpu_count(),
           "walk_is": "GS_BULGE_FORM=0: k_search_general (the parent commit's kernel plus the guide-list select), same process and box"}

    def save():
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(out, indent=1) + "\n")

    try:
        seqs_all, pams_all, _, _ = synth.sample_guides(h.text, args.guides, seed=77)
        for name, n, m in (("bulges_m1_rna1_dna1", args.guides, 1), ("bulges_m3_rna1_dna1", args.guides3, 3)):
            seqs, pams = seqs_all[:n], pams_all[:n]
            cfg = dict(mismatches=m, rna_bulges=1, dna_bulges=1)
            row = {"guides": n, **cfg, "forms": {}}
            h.gidx.set_option("GS_BULGE_FORM", 0)
            repeat = args.repeat if m == 1 else args.repeat3
            walk, secs = timed(h.gidx, seqs, pams, cfg, repeat)
            row["hits"] = int(walk[0][-1])
            row["forms"]["walk"] = {"seconds": [round(s, 4) for s in secs], "guides_per_s": n / min(secs),
                                    "general_last": h.gidx.general_last()}
            print(f"[bulge_bench] {name} walk: {row['forms']['walk']}", file=sys.stderr, flush=True)
            for rows in ((0, 8, 64, 512) if m == 1 else tuple(int(r) for r in args.rows3.split(","))):
                h.gidx.set_option("GS_BULGE_FORM", 1)
                h.gidx.set_option("GS_BULGE_ROWS", rows)
                got, secs = timed(h.gidx, seqs, pams, cfg, repeat)
                same = bool(np.array_equal(got[0], walk[0]) and got[1].tobytes() == walk[1].tobytes() and
                            np.array_equal(got[2], walk[2]))
                row["forms"][f"seeded_rows{rows}"] = {"seconds": [round(s, 4) for s in secs], "guides_per_s": n / min(secs),
                                                      "identical_to_walk": same,
                                                      "bulge_last": dict(zip(LAST, h.gidx.bulge_last()))}
                print(f"[bulge_bench] {name} seeded rows={rows}: {row['forms'][f'seeded_rows{rows}']}", file=sys.stderr,
                      flush=True)
            h.gidx.set_option("GS_BULGE_ROWS", None)
            out[name] = row
            save()
            if m == 1 and not args.skip_ref:
                n = min(args.ref_guides, args.guides)
                seqs, pams = seqs_all[:n], pams_all[:n]
                ids = [f"bul{i}" for i in range(n)]
                want, secs = gb.ref_lines(h, "bulges", [(ids[i], seqs[i].tobytes().decode(), "NGG") for i in range(n)], m, 1, 1)
                ref = {"guides": n, "reference_seconds": round(secs, 2), "lines": len(want)}
                for form in (0, 1):
                    h.gidx.set_option("GS_BULGE_FORM", form)
                    off, hx = h.gidx.enumerate_general(seqs, pams, mismatches=m, rna_bulges=1, dna_bulges=1)
                    got = []
                    for i in range(n):
                        got += api.format_guide_ex(h.gs, ids[i], seqs[i].tobytes().decode(), "NGG", True, hx[off[i]:off[i + 1]],
                                                   m).splitlines()
                    got.sort()
                    ref["identical_to_reference_" + ("seeded" if form else "walk")] = got == want
                out[name]["reference"] = ref
                save()
    finally:
        h.gidx.set_option("GS_BULGE_FORM", None)
        h.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""`guidescan enumerate --all-candidates --regions BED --pairs PAIRS.csv --max-span X ...`: PAIRS.csv must be the table
tests/pairs_model.py writes, and the database the file the oracle writes for the guides of the model's pairs, under both
encoders; SAM and --annotate run; every refusal prints one line and leaves no file.  GPU only."""
from types import SimpleNamespace

import pytest

import design_model as dm
import oracle_lib as ol
import pairs_model as pm
import test_oracle_vs_ref_pipeline as pipe
from test_cli_design_gpu import M, genomes, run   # noqa: F401 (genomes is a fixture)

pytestmark = pytest.mark.gpu

# name -> (command line, the model's rule, --per-region, --min-specificity, -t)
OPTION_SETS = {
    "any": (["--max-span", 60, "--per-region", 3], dict(max_span=60), 3, None, -1),
    "out_offset": (["--max-span", 300, "--min-span", 20, "--cut-offset", 0, "--pair-orientation", "pam-out", "--per-region", 2,
                    "--min-specificity", "0.3"], dict(max_span=300, min_span=20, cut_offset=0, orientation="pam-out"), 2, 0.3, -1),
    "all_in_t1": (["--max-span", 45, "--pair-orientation", "pam-in", "-t", 1], dict(max_span=45, orientation="pam-in"), None, None, 1),
}


def model_pairs(g, rule, per_region, min_specificity, threshold):
    groups, merged = dm.parse_bed(g["bed"].encode(), g["names"], g["lengths"])
    recs = dm.records(groups, merged, g["chromosomes"], "NGG", 20)
    dm.score(recs, g["oidx"], g["lengths"], "NGG", mismatches=M, threshold=threshold)
    kept = pm.pairs(recs, 20, 3, per_region=per_region, min_specificity=min_specificity, **rule)
    sel, _ = pm.guides(recs, kept)
    return groups, recs, kept, sel


@pytest.mark.parametrize("genome", ["planted", "toy"])
@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_the_table_is_the_model_s_and_the_database_the_oracle_s(genomes, genome, name):
    g = genomes[genome]
    args, rule, n, s, thr = OPTION_SETS[name]
    groups, recs, kept, sel = model_pairs(g, rule, n, s, thr)
    assert kept and 2 <= len(sel) < len(recs)
    table = pm.table(recs, kept, groups, g["names"], 20, 3, rule.get("cut_offset", 3)).encode()
    kmers = [SimpleNamespace(id=i, sequence=r["seq"], pam="NGG", positive=r["sense"] == "+")
             for i, r in zip(dm.ids(sel, groups, g["names"]), sel)]
    want = pipe.oracle_file(g["oidx"], g["names"], g["lengths"], kmers, fmt="csv", m=M, thr=thr)
    base = ["enumerate", g["prefix"], "--all-candidates", "--regions", g["bed_path"], "-m", M, "-n", "1", "--verbose"]
    for encoder in ("host", "gpu"):
        out, pairs = g["work"] / f"pairs_{genome}_{name}_{encoder}.csv", g["work"] / f"pairs_{genome}_{name}_{encoder}.pairs.csv"
        r = run(base + ["--encoder", encoder, "-o", out, "--pairs", pairs] + args)
        assert r.returncode == 0, r.stderr
        assert pairs.read_bytes() == table, encoder
        assert out.read_bytes() == want, encoder
        in_groups = len({recs[a]["group"] for a, _ in kept})
        assert f"Paired {len(kept)} pair(s) of {len(sel)} guide(s) in {in_groups} group(s)" in r.stdout and "Pairs:" in r.stdout
        assert "Selected" not in r.stdout
    if name == "any":
        sam, pairs = g["work"] / f"pairs_{genome}.sam", g["work"] / f"pairs_{genome}_sam.pairs.csv"
        r = run(base + ["--format", "sam", "--encoder", "gpu", "-o", sam, "--pairs", pairs] + args)
        assert r.returncode == 0, r.stderr
        assert pairs.read_bytes() == table
        assert sam.read_bytes() == pipe.oracle_file(g["oidx"], g["names"], g["lengths"], kmers, fmt="sam", m=M)
        # with --annotate the database gains a column; the table is what it was
        ann, pairs = g["work"] / f"pairs_{genome}_annot.csv", g["work"] / f"pairs_{genome}_annot.pairs.csv"
        r = run(base + ["--annotate", g["bed_path"], "-o", ann, "--pairs", pairs] + args)
        assert r.returncode == 0, r.stderr
        assert pairs.read_bytes() == table
        lines = ann.read_text().splitlines()
        assert lines[0].endswith(",match_features") and len(lines) == want.count(b"\n")


def test_refusals(genomes, toy):
    g = genomes["planted"]
    out, pairs = g["work"] / "pairs_refused.csv", g["work"] / "pairs_refused.pairs.csv"
    base = ["enumerate", g["prefix"], "-o", out, "--pairs", pairs]
    scan = base + ["--all-candidates", "--regions", g["bed_path"]]
    cases = [
        (base + ["--all-candidates", "--max-span", 40], "--pairs pairs the guides within the groups of"),
        (base + ["-f", toy["dir"] / "kmers.csv", "--max-span", 40], "--pairs pairs the guides within the groups of"),
        (scan, "--pairs needs --max-span"),
        (["enumerate", g["prefix"], "-o", out, "--all-candidates", "--regions", g["bed_path"], "--max-span", 40], "describe the pairs of --pairs"),
        (["enumerate", g["prefix"], "-o", out, "--all-candidates", "--regions", g["bed_path"], "--min-span", 4], "describe the pairs of --pairs"),
        (["enumerate", g["prefix"], "-o", out, "--all-candidates", "--regions", g["bed_path"], "--cut-offset", 4], "describe the pairs of --pairs"),
        (["enumerate", g["prefix"], "-o", out, "--all-candidates", "--regions", g["bed_path"], "--pair-orientation", "any"],
         "describe the pairs of --pairs"),
        (scan + ["--max-span", "4x"], "--max-span 4x: a number"),
        (scan + ["--max-span", "-4"], "--max-span -4: a number"),
        (scan + ["--max-span", 40, "--min-span", "two"], "--min-span two: a number"),
        (scan + ["--max-span", 40, "--cut-offset", "3.5"], "--cut-offset 3.5: a number"),
        (scan + ["--max-span", 40, "--pair-orientation", "sideways"], "--pair-orientation sideways"),
        (scan + ["--max-span", 40, "--min-span", 41], "--min-span is larger than --max-span"),
        (scan + ["--max-span", 40, "--cut-offset", 21], "--cut-offset lies beyond the k-mer length"),
        (scan + ["--max-span", 40, "--kmer-length", 18, "--cut-offset", 19], "--cut-offset lies beyond the k-mer length"),
        (scan + ["--max-span", 40, "--rna-bulges", 1], "--pairs scores on the fast path"),
        (scan + ["--max-span", 40, "-m", 8], "--pairs scores on the fast path"),
        (scan + ["--max-span", 40, "-a", "NGAG"], "--pairs scores on the fast path"),
        (scan + ["--max-span", 40, "--pam", "TTTN", "--kmer-length", 26, "--start"], "--pairs scores on the fast path"),
        (["kmers", g["prefix"], "-o", out, "--regions", g["bed_path"], "--pairs", pairs], "takes the index"),
    ]
    for args, message in cases:
        r = run(args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
        assert r.stderr.count("\n") == 1, (args, r.stderr)
        assert not out.exists() and not pairs.exists()


def test_the_help_lists_the_options():
    r = run(["enumerate", "--help"])
    for option in ("--pairs", "--max-span", "--min-span", "--cut-offset", "--pair-orientation"):
        assert option in r.stderr

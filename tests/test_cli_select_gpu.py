"""`guidescan kmers` and `guidescan enumerate --all-candidates` with the sequence rules (--gc, --max-run, --exclude-motif,
--exclude-site) and `--regions BED --per-region N --min-spacing D`: the kmers file must hold the rows tests/select_model.py
keeps, the database exactly the ids the model picks, under both encoders; the report lines are the model's counts; every
refusal is one line, a non-zero exit and nothing written.  GPU only."""
import pytest

import design_cases as dc
import design_model as dm
import select_model as sl
from test_cli_design_gpu import M, genomes, run   # noqa: F401 (genomes is a fixture)

pytestmark = pytest.mark.gpu

RULE_ARGS = ["--gc", "40:70", "--max-run", 3, "--exclude-site", "CGTCTC"]
RULE = dict(gc=(40, 70), max_run=3, exclude_sites=("CGTCTC",))
HEADER = "id,sequence,pam,chromosome,position,sense\n"


def rule_line(counts):
    kept = counts["scanned"] - counts["gc"] - counts["run"] - counts["motif"]
    return (f"Sequence rules: kept {kept} of {counts['scanned']} candidate(s); {counts['gc']} failed --gc, {counts['run']} --max-run, "
            f"{counts['motif']} a motif\n")


def passes(seq, rule):
    return sl.charge(seq, rule.get("gc"), rule.get("max_run"), sl.motif_list(rule.get("exclude_motifs", ()), rule.get("exclude_sites", ()))) == sl.PASS


def test_kmers_with_the_rules_genome_wide(genomes):
    g = genomes["planted"]
    for args, rule in ((RULE_ARGS, RULE), (["--exclude-motif", "TTTT,GGNCC"], dict(exclude_motifs=("TTTT", "GGNCC")))):
        rows, total = [HEADER], dict(scanned=0, gc=0, run=0, motif=0)
        for (c, _), cands in zip(g["chromosomes"], dc.candidates()):
            kept, counts, _ = sl.filter_candidates(cands, **rule)
            rows += [f"{g['names'][c]}:{p}:{s},{q},NGG,{g['names'][c]},{p},{s}\n" for q, p, s in kept]
            total = {k: total[k] + counts[k] for k in total}
        out = g["work"] / "select_kmers.csv"
        r = run(["kmers", g["prefix"], "-o", out] + args)
        assert r.returncode == 0, r.stderr
        assert out.read_text() == "".join(rows) and 1 < len(rows) < 1186
        assert rule_line(total) in r.stdout and f"Wrote {len(rows) - 1} candidate(s)" in r.stdout


def test_kmers_with_the_rules_and_regions(genomes):
    g = genomes["planted"]
    groups, recs = dc.model_records(g["bed"])
    sel = dm.select([r for r in recs if passes(r["seq"], RULE)])
    assert 0 < len(sel) < len(recs)
    out = g["work"] / "select_kmers_regions.csv"
    r = run(["kmers", g["prefix"], "-o", out, "--regions", g["bed_path"]] + RULE_ARGS)
    assert r.returncode == 0, r.stderr
    assert out.read_text() == HEADER + dm.rows(sel, groups, g["names"], "NGG")
    total = dict(scanned=0, gc=0, run=0, motif=0)
    for cands in dc.candidates():
        counts = sl.filter_candidates(cands, **RULE)[1]
        total = {k: total[k] + counts[k] for k in total}
    assert rule_line(total) in r.stdout and total["scanned"] == 1185


def test_enumerate_picks_the_model_s_ids(genomes):
    g = genomes["planted"]
    groups, recs = dc.model_records(g["bed"])
    recs = [r for r in recs if passes(r["seq"], RULE)]
    dm.score(recs, g["oidx"], g["lengths"], "NGG", mismatches=M)
    sel, spacing = sl.select_spaced(recs, 3, 25, 20, 3)
    unspaced = dm.select(recs, 3)
    ids = dm.ids(sel, groups, g["names"])
    assert ids != dm.ids(unspaced, groups, g["names"]) and spacing["passed_over"] > 0
    total = dict(scanned=0, gc=0, run=0, motif=0)
    for cands in dc.candidates():
        counts = sl.filter_candidates(cands, **RULE)[1]
        total = {k: total[k] + counts[k] for k in total}
    for encoder in ("host", "gpu"):
        out = g["work"] / f"select_{encoder}.csv"
        r = run(["enumerate", g["prefix"], "--all-candidates", "--regions", g["bed_path"], "--per-region", 3, "--min-spacing", 25, "-m", M,
                 "--encoder", encoder, "-n", "1", "--verbose", "-o", out] + RULE_ARGS)
        assert r.returncode == 0, r.stderr
        got = []
        for line in out.read_text().splitlines()[1:]:
            if line.split(",")[0] not in got:
                got.append(line.split(",")[0])
        assert got == ids, encoder
        assert rule_line(total) in r.stdout
        assert f"Selected {len(sel)} guide(s) of {len(recs)} record(s)" in r.stdout and "Regions:" in r.stdout
        assert (f"Spacing: {spacing['passed_over']} record(s) passed over within 25 base(s) of a pick, "
                f"{spacing['groups_short_for_spacing']} group(s) short of --per-region for it") in r.stdout
    # without --regions the rules still drop candidates before the search: every id left passes them
    out = g["work"] / "select_all.csv"
    r = run(["enumerate", g["prefix"], "--all-candidates", "-m", 0, "-n", "1", "-o", out, "--chromosomes", g["names"][1]] + RULE_ARGS)
    assert r.returncode == 0, r.stderr
    kept = sl.filter_candidates(dc.candidates()[1], **RULE)[0]
    seen = []
    for line in out.read_text().splitlines()[1:]:
        if line.split(",")[0] not in seen:
            seen.append(line.split(",")[0])
    assert seen == [f"{g['names'][1]}:{p}:{s}" for _, p, s in kept] and "Sequence rules: kept" in r.stdout


def test_refusals(genomes, toy):
    g = genomes["planted"]
    out, pairs = g["work"] / "select_refused.csv", g["work"] / "select_refused.pairs.csv"
    scan = ["enumerate", g["prefix"], "-o", out, "--all-candidates", "--regions", g["bed_path"]]
    cases = [
        (scan + ["--min-spacing", 25], "--min-spacing needs --per-region"),
        (scan + ["--min-spacing", 25, "--per-region", 1025], "--min-spacing needs --per-region"),
        (scan + ["--min-spacing", 25, "--per-region", 3, "--pairs", pairs, "--max-span", 60], "--min-spacing spaces single guides"),
        (["enumerate", g["prefix"], "-o", out, "--all-candidates", "--per-region", 3, "--min-spacing", 25], "--min-spacing spaces the picks within"),
        (scan + ["--min-spacing", 25, "--per-region", 3, "--cut-offset", 21], "--cut-offset lies beyond the k-mer length"),
        (scan + ["--min-spacing", "x"], "--min-spacing x: a number"),
        (["enumerate", g["prefix"], "-o", out, "-f", toy["dir"] / "kmers.csv", "--gc", "40:70"], "the user's own choice of guides"),
        (["enumerate", g["prefix"], "-o", out, "-f", toy["dir"] / "kmers.csv", "--exclude-motif", "TTTT"], "the user's own choice of guides"),
        (scan + ["--exclude-motif", "ACXT"], "motif 'ACXT'"),
        (scan + ["--exclude-site", "ACGT,,A"], "motif ''"),
        (scan + ["--exclude-motif", ",".join(["A"] * 17)], "more than 16 motifs"),
        (scan + ["--exclude-motif", "A" * 33], "more than 32 letters"),
        (scan + ["--gc", "70:40"], "--gc 70:40: MIN:MAX"),
        (scan + ["--gc", "40"], "--gc 40: MIN:MAX"),
        (scan + ["--gc", "40:101"], "--gc 40:101: MIN:MAX"),
        (scan + ["--max-run", 0], "--max-run 0:"),
        (["kmers", g["prefix"], "-o", out, "--exclude-motif", "ACXT"], "motif 'ACXT'"),
        (["kmers", g["prefix"], "-o", out, "--gc", "70:40"], "--gc 70:40: MIN:MAX"),
        (["kmers", g["prefix"], "-o", out, "--regions", g["bed_path"], "--min-spacing", 5], "takes the index"),
    ]
    for args, message in cases:
        r = run(args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
        assert r.stderr.count("\n") == 1, (args, r.stderr)
        assert not out.exists() and not pairs.exists()


def test_the_help_lists_the_options():
    r = run(["enumerate", "--help"])
    for option in ("--gc", "--max-run", "--exclude-motif", "--exclude-site", "--min-spacing"):
        assert option in r.stderr

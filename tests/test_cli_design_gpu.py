"""`guidescan enumerate --all-candidates --regions BED [--per-region N] [--min-specificity S]` and `guidescan kmers
--regions BED`: the database must be the file the oracle writes for the kmers file that tests/design_model.py selects
(and the compiled reference's, where oracle/_ref is built), in CSV and SAM, under both encoders; the BAM of --bgzf gpu
must hold the SAM's records; the refusals print their message; without --regions nothing changes.  GPU only."""
import os
import subprocess
from types import SimpleNamespace

import pytest

import bam_reader
import design_cases as dc
import design_model as dm
import oracle_lib as ol
import test_oracle_vs_ref_pipeline as pipe
from test_cli_bgzf_gpu import starred
from test_design_model import assert_cases_decide, closing_up

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
live = pipe.ref is not None and pipe.SHIM.exists()
M = dc.MISMATCHES


def run(args):
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)


def toy_bed(names, lengths):
    """two groups on the first chromosome, nested, the second also on the last chromosome"""
    a, z = names[0], names[-1]
    return (f"{a}\t0\t{min(lengths[0], 700)}\touter\n{a}\t100\t{min(lengths[0], 400)}\tinner\n"
            f"{z}\t{max(0, lengths[-1] - 500)}\t{lengths[-1]}\tinner\n")


@pytest.fixture(scope="module")
def genomes(toy, tmp_path_factory):
    """name -> dict(prefix, text, names, lengths, chromosomes, bed path, bed text, oracle index)"""
    work = tmp_path_factory.mktemp("design")
    text, names, lengths, chromosomes = dc.genome()
    fa = work / "planted.fa"
    with open(fa, "wb") as f:
        for (c, chrm), n in zip(chromosomes, names):
            f.write(b">" + n.encode() + b"\n" + chrm + b"\n")
    out = {"planted": dict(fa=fa, text=text, names=names, lengths=lengths, chromosomes=chromosomes, bed=dc.selection_bed())}
    begin = [0]
    for ln in toy["lengths"]:
        begin.append(begin[-1] + int(ln))
    tl = [int(x) for x in toy["lengths"]]
    out["toy"] = dict(fa=toy["dir"] / "toy.fa", text=toy["text"], names=list(toy["names"]), lengths=tl,
                      chromosomes=[(i, toy["text"][begin[i]:begin[i + 1]].tobytes()) for i in range(len(tl))],
                      bed=toy_bed(list(toy["names"]), tl))
    for name, g in out.items():
        g["prefix"] = work / name
        r = run(["index", "--index", g["prefix"], g["fa"]])
        assert r.returncode == 0, r.stderr
        g["bed_path"] = work / f"{name}.bed"
        g["bed_path"].write_text(g["bed"])
        g["oidx"] = ol.OracleIndex(g["text"])
        g["work"] = work
    yield out
    for g in out.values():
        g["oidx"].close()


OPTION_SETS = {
    "regions": dict(),
    "per_region": dict(per_region=2),
    "per_region_min_nag": dict(per_region=3, min_specificity=0.6, alt=("NAG",)),
}


def model_selection(g, per_region=None, min_specificity=None, alt=(), threshold=-1):
    groups, merged = dm.parse_bed(g["bed"].encode(), g["names"], g["lengths"])
    recs = dm.records(groups, merged, g["chromosomes"], "NGG", 20)
    if per_region is not None or min_specificity is not None or threshold > 0:
        dm.score(recs, g["oidx"], g["lengths"], "NGG", mismatches=M, alt_pams=alt, threshold=threshold)
    sel = dm.select(recs, per_region, min_specificity)
    return groups, sel


def cli_options(cfg):
    o = []
    if "per_region" in cfg:
        o += ["--per-region", cfg["per_region"]]
    if "min_specificity" in cfg:
        o += ["--min-specificity", cfg["min_specificity"]]
    for a in cfg.get("alt", ()):
        o += ["-a", a]
    return o


@pytest.mark.parametrize("genome", ["planted", "toy"])
@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_the_database_is_the_oracle_s_for_the_model_s_kmers(genomes, genome, name):
    g, cfg = genomes[genome], OPTION_SETS[name]
    groups, sel = model_selection(g, cfg.get("per_region"), cfg.get("min_specificity"), cfg.get("alt", ()))
    assert len(sel) >= 1
    ids = dm.ids(sel, groups, g["names"])
    kmers = [SimpleNamespace(id=i, sequence=r["seq"], pam="NGG", positive=r["sense"] == "+") for i, r in zip(ids, sel)]
    for fmt in ("csv", "sam"):
        want = pipe.oracle_file(g["oidx"], g["names"], g["lengths"], kmers, fmt=fmt, m=M, alt=cfg.get("alt", ()))
        for encoder in ("host", "gpu"):
            out = g["work"] / f"{genome}_{name}_{encoder}.{fmt}"
            r = run(["enumerate", g["prefix"], "--all-candidates", "--regions", g["bed_path"], "-m", M, "--format", fmt,
                     "--encoder", encoder, "-n", "1", "--verbose", "-o", out] + cli_options(cfg))
            assert r.returncode == 0, r.stderr
            assert out.read_bytes() == want, (fmt, encoder)
            assert f"Selected {len(sel)} guide(s)" in r.stdout and "Regions:" in r.stdout
    if live and name == "per_region" and genome == "planted":
        kcsv = g["work"] / "model_kmers.csv"
        kcsv.write_text("id,sequence,pam,chromosome,position,sense\n" + dm.rows(sel, groups, g["names"], "NGG"))
        pipe.write_reference_index(g["oidx"], g["text"].shape[0] + 1, g["work"] / "refidx", g["names"], g["lengths"])
        assert pipe.run_shim(g["work"] / "refidx", kcsv, g["work"] / "ref.csv", m=M) == \
            (g["work"] / f"{genome}_{name}_gpu.csv").read_bytes()
    # the BAM of --bgzf gpu holds the SAM's records
    bam = g["work"] / f"{genome}_{name}.bam"
    r = run(["enumerate", g["prefix"], "--all-candidates", "--regions", g["bed_path"], "-m", M, "--format", "bam", "--bgzf", "gpu",
             "-o", bam] + cli_options(cfg))
    assert r.returncode == 0, r.stderr
    assert bam_reader.to_sam(bam) == starred((g["work"] / f"{genome}_{name}_gpu.sam").read_text())


def test_threshold_drops_before_the_ranking(genomes):
    g = genomes["planted"]
    groups, merged = dm.parse_bed(g["bed"].encode(), g["names"], g["lengths"])
    recs = dm.records(groups, merged, g["chromosomes"], "NGG", 20)
    dm.score(recs, g["oidx"], g["lengths"], "NGG", mismatches=M, threshold=1)
    assert_cases_decide(groups, recs)   # S = 0.6 of the option sets above splits a group; -t 1 drops records
    n = closing_up(recs)   # the first N at which a record made ineligible changes who is among a group's first N
    assert n is not None
    sel = dm.select(recs, per_region=n)
    kmers = [SimpleNamespace(id=i, sequence=r["seq"], pam="NGG", positive=r["sense"] == "+")
             for i, r in zip(dm.ids(sel, groups, g["names"]), sel)]
    want = pipe.oracle_file(g["oidx"], g["names"], g["lengths"], kmers, fmt="csv", m=M, thr=1)
    out = g["work"] / "threshold.csv"
    r = run(["enumerate", g["prefix"], "--all-candidates", "--regions", g["bed_path"], "-m", M, "-t", 1, "--per-region", n,
             "--encoder", "gpu", "-o", out])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == want


def test_threshold_without_a_selection_is_the_pipeline_s_own_pass(genomes):
    """--regions -t 1 and nothing else: no score phase (no index is needed to pick the guides), the records go to the
    batch pipeline and its threshold pass drops what the reference drops - on the route of bulges too"""
    g = genomes["planted"]
    groups, sel = model_selection(g)
    kmers = [SimpleNamespace(id=i, sequence=r["seq"], pam="NGG", positive=r["sense"] == "+")
             for i, r in zip(dm.ids(sel, groups, g["names"]), sel)]
    for tag, extra, kw in (("plain", [], {}), ("bulge", ["--rna-bulges", 1], dict(rna=1))):
        want = pipe.oracle_file(g["oidx"], g["names"], g["lengths"], kmers, fmt="csv", m=1, thr=1, **kw)
        assert want.count(b"\n") > 10
        out = g["work"] / f"threshold_only_{tag}.csv"
        r = run(["enumerate", g["prefix"], "--all-candidates", "--regions", g["bed_path"], "-m", 1, "-t", 1, "-o", out] + extra)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == want, tag


@pytest.mark.parametrize("genome", ["planted", "toy"])
def test_kmers_regions_writes_the_model_s_rows(genomes, genome):
    g = genomes[genome]
    groups, sel = model_selection(g)
    out = g["work"] / f"{genome}.regions.kmers.csv"
    r = run(["kmers", g["prefix"], "--regions", g["bed_path"], "--prefix", "lib_", "-o", out])
    assert r.returncode == 0, r.stderr
    assert out.read_text() == "id,sequence,pam,chromosome,position,sense\n" + dm.rows(sel, groups, g["names"], "NGG", "lib_")
    assert f"Wrote {len(sel)} candidate(s)" in r.stdout


def test_refusals(genomes, toy):
    g = genomes["planted"]
    out = g["work"] / "refused.csv"
    base = ["enumerate", g["prefix"], "-o", out]
    cases = [
        (base + ["-f", toy["dir"] / "kmers.csv", "--regions", g["bed_path"]], "--regions restricts the scan of --all-candidates"),
        (base + ["--all-candidates", "--per-region", 2], "--per-region and --min-specificity select within the groups of --regions"),
        (base + ["--all-candidates", "--min-specificity", "0.5"], "--per-region and --min-specificity select within the groups of --regions"),
        (base + ["--all-candidates", "--regions", g["bed_path"], "--per-region", 0], "--per-region 0"),
        (base + ["--all-candidates", "--regions", g["bed_path"], "--min-specificity", "1.5"], "--min-specificity 1.5"),
        (base + ["--all-candidates", "--regions", g["bed_path"], "--min-specificity", "0.5x"], "--min-specificity 0.5x"),
        (base + ["--all-candidates", "--regions", g["work"] / "missing.bed"], "cannot read the regions file"),
        (["kmers", g["prefix"], "-o", out, "--regions", g["bed_path"], "--per-region", 2], "takes the index"),
        (["kmers", g["prefix"], "-o", out, "--min-specificity", "0.2"], "takes the index"),
    ]
    bad = g["work"] / "bad.bed"
    bad.write_text(f"{g['names'][0]}\t0\t100\tok\n{g['names'][0]}\t50\t40\tg\n")
    cases.append((base + ["--all-candidates", "--regions", bad], "regions line 2: start >= end"))
    cases.append((["kmers", g["prefix"], "-o", out, "--regions", bad], "regions line 2: start >= end"))
    wide = base + ["--all-candidates", "--regions", g["bed_path"], "--per-region", 2, "--pam", "TTTN", "--kmer-length", 26, "--start"]
    cases.append((wide, "scores on the fast path"))
    for args, message in cases:
        r = run(args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
        assert not out.exists()


def test_without_regions_nothing_changes(genomes):
    """the same bytes as `enumerate -f` on the kmers file of `guidescan kmers`: the route the existing tests pin"""
    g = genomes["planted"]
    k = g["work"] / "all.kmers.csv"
    assert run(["kmers", g["prefix"], "-o", k]).returncode == 0
    a, b = g["work"] / "all_f.csv", g["work"] / "all_scan.csv"
    assert run(["enumerate", g["prefix"], "-f", k, "-m", M, "-o", a]).returncode == 0
    r = run(["enumerate", g["prefix"], "--all-candidates", "--encoder", "gpu", "-m", M, "-o", b])
    assert r.returncode == 0 and "Selected" not in r.stdout
    assert a.read_bytes() == b.read_bytes() and a.stat().st_size > 10_000

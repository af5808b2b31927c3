"""`guidescan enumerate --annotate BED [--max-feature-hits K [--feature-distance D]]`: the CSV gets one more column and
nothing else changes; the column is the one tests/annot_model.py gives each row; the selection rule names the guides the
model selects; the refusals print their message.  GPU only."""
import os
import subprocess

import pytest

import annot_cases as ac
import design_cases as dc
import design_model as dm
import oracle_lib as ol
from test_annot_model import dup_bed, feature_hits_model

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
M = dc.MISMATCHES


def run(args, **env_more):
    env = dict(os.environ, **env_more)
    env.pop("GS_ENCODER", None)
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    work = tmp_path_factory.mktemp("annotate")
    text, names, lengths, chromosomes = dc.genome()
    fa = work / "planted.fa"
    with open(fa, "wb") as f:
        for (c, chrm), n in zip(chromosomes, names):
            f.write(b">" + n.encode() + b"\n" + chrm + b"\n")
    prefix = work / "planted"
    r = run(["index", "--index", prefix, fa])
    assert r.returncode == 0, r.stderr
    bed = work / "cases.bed"
    bed.write_text(ac.case_bed())
    kmers = work / "all.kmers.csv"
    assert run(["kmers", prefix, "-o", kmers]).returncode == 0
    # a kmers file whose first batch falls back from --encoder gpu to the host route: one guide is not over A,C,G,T
    rows = kmers.read_text().splitlines()
    mixed = work / "mixed.kmers.csv"
    odd = rows[5].split(",")
    odd[0], odd[1] = "odd", odd[1][:7] + "N" + odd[1][8:]
    mixed.write_text("\n".join(rows[:300] + [",".join(odd)] + rows[300:600]) + "\n")
    return dict(work=work, prefix=prefix, bed=bed, kmers=kmers, mixed=mixed, names=names, lengths=lengths, text=text)


def check_pair(with_column, plain):
    """the annotated file against the plain one and the model -> the column"""
    h1, _, body1 = with_column.partition(b"\n")
    h0, _, body0 = plain.partition(b"\n")
    assert h1 == h0 + b",match_features"
    return ac.check_text(body1, body0, ac.case_bed())


SOURCES = {"file": lambda g: ["-f", g["kmers"]], "scan": lambda g: ["--all-candidates"]}


@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("mode", ["complete", "succinct"])
def test_one_more_column_and_nothing_else(planted, source, mode):
    g = planted
    files = {}
    for encoder in ("host", "gpu"):
        for annotate in (False, True):
            out = g["work"] / f"{source}_{mode}_{encoder}_{int(annotate)}.csv"
            r = run(["enumerate", g["prefix"], "-m", M, "--mode", mode, "--encoder", encoder, "-o", out] + SOURCES[source](g) +
                    (["--annotate", g["bed"]] if annotate else []))
            assert r.returncode == 0, r.stderr
            assert ("Annotation: " in r.stdout) == annotate
            if encoder == "gpu":
                assert "Encoder: gpu (1 batch(es) encoded on the device, 0 by the host encoders)" in r.stdout
            files[encoder, annotate] = out.read_bytes()
    assert files["host", False] == files["gpu", False]
    assert files["host", True] == files["gpu", True]
    col = check_pair(files["gpu", True], files["gpu", False])
    assert len(col) > 1000 and "NA" in col and any(c.count(";") >= 299 for c in col) and "gene;exon0" in col


def test_the_other_routes_write_the_same_bytes(planted):
    """--kmers gpu, two workers, small batches, a capped --max-off-targets; a batch that falls back to the host encoders"""
    g = planted
    base = ["enumerate", g["prefix"], "-m", M, "--annotate", g["bed"]]
    want = g["work"] / "routes_want.csv"
    assert run(base + ["-f", g["kmers"], "-o", want]).returncode == 0
    for tag, extra, env in (("kmers_gpu", ["--kmers", "gpu", "--encoder", "gpu"], {}),
                            ("two_workers", ["--gpus", 2, "--batch-size", 256, "--encoder", "gpu"], {"GS_CLI_SAME_DEVICE": "1"}),
                            ("two_workers_host", ["--gpus", 2, "--batch-size", 256], {"GS_CLI_SAME_DEVICE": "1"})):
        out = g["work"] / f"routes_{tag}.csv"
        r = run(base + ["-f", g["kmers"], "-o", out] + extra, **env)
        assert r.returncode == 0, (tag, r.stderr)
        assert out.read_bytes() == want.read_bytes(), tag
    capped = {}
    for encoder in ("host", "gpu"):
        for annotate in (False, True):
            out = g["work"] / f"capped_{encoder}_{int(annotate)}.csv"
            r = run(["enumerate", g["prefix"], "-m", M, "--max-off-targets", 1, "-f", g["kmers"], "--encoder", encoder, "-o", out] +
                    (["--annotate", g["bed"]] if annotate else []))
            assert r.returncode == 0, r.stderr
            capped[encoder, annotate] = out.read_bytes()
    assert capped["host", True] == capped["gpu", True]
    check_pair(capped["gpu", True], capped["gpu", False])
    mixed = {}
    for encoder in ("host", "gpu"):
        out = g["work"] / f"mixed_{encoder}.csv"
        r = run(base + ["-f", g["mixed"], "--encoder", encoder, "-o", out])
        assert r.returncode == 0, r.stderr
        mixed[encoder] = out.read_bytes()
        if encoder == "gpu":
            assert "0 batch(es) encoded on the device, 1 by the host encoders" in r.stdout
    assert mixed["host"] == mixed["gpu"] and b"\nodd," in mixed["gpu"]
    plain = g["work"] / "mixed_plain.csv"
    assert run(["enumerate", g["prefix"], "-m", M, "-f", g["mixed"], "-o", plain]).returncode == 0
    check_pair(mixed["gpu"], plain.read_bytes())


def test_the_feature_rule_names_the_guides_the_model_selects(planted):
    g = planted
    regions, features = g["work"] / "selection.bed", g["work"] / "dup.bed"
    regions.write_text(dc.selection_bed())
    features.write_text(dup_bed())
    _, _, _, chromosomes = dc.genome()
    groups, merged = dm.parse_bed(dc.selection_bed().encode(), g["names"], g["lengths"])
    recs = dm.records(groups, merged, chromosomes, "NGG", 20)
    oidx = ol.OracleIndex(g["text"])
    dm.score(recs, oidx, g["lengths"], "NGG", mismatches=M)
    feature_hits_model(recs, oidx, M)
    near = feature_hits_model([dict(r) for r in recs], oidx, 0)
    oidx.close()
    # the issue's command; then the rule alone, where it must decide something; then within distance 0
    for tag, model, per_region, extra in (("top2", recs, 2, []), ("all", recs, None, []), ("d0", near, None, ["--feature-distance", 0])):
        sel = dm.select([dict(r, eligible=r["feature_hits"] == 0) for r in model], per_region=per_region)
        want = dm.ids(sel, groups, g["names"])
        if per_region is None:
            assert len(sel) < len(model) and any(r["feature_hits"] for r in model)
        for encoder in ("host", "gpu"):
            out = g["work"] / f"rule_{tag}_{encoder}.csv"
            r = run(["enumerate", g["prefix"], "--all-candidates", "--regions", regions, "--annotate", features, "--max-feature-hits", 0,
                     "-m", M, "--encoder", encoder, "-o", out] + (["--per-region", per_region] if per_region else []) + extra)
            assert r.returncode == 0, r.stderr
            got = []
            for row in out.read_text().splitlines()[1:]:
                if not got or got[-1] != row.split(",")[0]:
                    got.append(row.split(",")[0])
            assert got == want, (tag, encoder)
            assert f"Selected {len(sel)} guide(s)" in r.stdout


def test_refusals(planted):
    g = planted
    out = g["work"] / "refused.out"
    base = ["enumerate", g["prefix"], "-f", g["kmers"], "-o", out]
    bad = g["work"] / "bad.bed"
    bad.write_text(f"{g['names'][0]}\t0\t100\tok\n{g['names'][0]}\t50\t40\tg\n")
    semi = g["work"] / "semi.bed"
    semi.write_text(f"{g['names'][0]}\t0\t100\tgene;exon\n")
    scan = ["enumerate", g["prefix"], "--all-candidates", "-o", out]
    cases = [
        (base + ["--annotate", g["bed"], "--format", "sam"], "--annotate adds a column to the CSV database; --format sam has none"),
        (base + ["--annotate", g["bed"], "--format", "bam"], "--annotate adds a column to the CSV database; --format bam has none"),
        (base + ["--annotate", bad], "annotation line 2: start >= end"),
        (base + ["--annotate", g["work"] / "missing.bed"], "cannot read the annotation file"),
        (base + ["--annotate", semi], "gene;exon"),
        (scan + ["--annotate", g["bed"], "--max-feature-hits", 0], "--max-feature-hits selects among the candidates of --regions"),
        (scan + ["--regions", g["bed"], "--max-feature-hits", 0], "--max-feature-hits selects among the candidates of --regions"),
        (scan + ["--regions", g["bed"], "--annotate", g["bed"], "--feature-distance", 1], "--feature-distance is the distance"),
        (scan + ["--regions", g["bed"], "--annotate", g["bed"], "--max-feature-hits", "x"], "--max-feature-hits x"),
    ]
    for args, message in cases:
        r = run(args)
        assert r.returncode != 0 and message in r.stderr, (args, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1 or "usage" in r.stderr.lower() or "guidescan " in r.stderr
        assert not out.exists()
    # the SAM refusal comes before the index is loaded: no line of progress was printed
    r = run(base + ["--annotate", g["bed"], "--format", "sam"])
    assert r.stdout == "" and len(r.stderr.strip().splitlines()) == 1


def test_without_annotate_the_bytes_are_the_oracle_s(planted):
    """the route the existing CLI tests pin, on this genome: `enumerate -f` against the CPU oracle's file"""
    import test_oracle_vs_ref_pipeline as pipe
    from types import SimpleNamespace
    g = planted
    rows = [r.split(",") for r in g["kmers"].read_text().splitlines()[1:201]]
    some = g["work"] / "some.kmers.csv"
    some.write_text("id,sequence,pam,chromosome,position,sense\n" + "\n".join(",".join(r) for r in rows) + "\n")
    kmers = [SimpleNamespace(id=r[0], sequence=r[1], pam=r[2], positive=r[5] == "+") for r in rows]
    oidx = ol.OracleIndex(g["text"])
    for fmt in ("csv", "sam"):
        want = pipe.oracle_file(oidx, g["names"], g["lengths"], kmers, fmt=fmt, m=M)
        for encoder in ("host", "gpu"):
            out = g["work"] / f"plain_{encoder}.{fmt}"
            assert run(["enumerate", g["prefix"], "-f", some, "-m", M, "--format", fmt, "--encoder", encoder, "-o", out]).returncode == 0
            assert out.read_bytes() == want, (fmt, encoder)
    oidx.close()

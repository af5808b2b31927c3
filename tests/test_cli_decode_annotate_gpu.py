"""`guidescan decode --annotate BED [--features-only]`: the table is the one the command prints without the option plus
the columns tests/annot_model.py gives each row (tests/decode_annot_cases.py); SAM and BAM input, --bgzf host and gpu,
--fasta host and gpu, -o and stdout, small batches; the two usage errors; a malformed BED line ends as it ends
`enumerate --annotate`.  GPU only."""
import subprocess

import pytest

import bam_make as bm
import decode_annot_cases as dac
import decode_golden as dg
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"


def run(args, **kw):
    return subprocess.run([str(CLI)] + [str(a) for a in args], timeout=300, capture_output=True, **kw)


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_annotate")
    recs = dac.small_records()
    sam = dac.sam_text(recs)
    (d / "db.sam").write_text(sam)
    head, records = bm.from_sam(sam)
    (d / "db.bam").write_bytes(b"".join(bm.members(head + b"".join(records), piece=900)) + bm.EOF_BLOCK)
    dac.write_fasta(d / "g.fa", dac.small_genome())
    (d / "f.bed").write_text(dac.small_bed())
    plain = {}
    for mode in dg.MODES:
        r = run(["decode", "--mode", mode, d / "db.sam", d / "g.fa"])
        assert r.returncode == 0, r.stderr
        plain[mode] = r.stdout
    bed = dac.small_bed()
    want = {"complete": dac.expected_complete(plain["complete"], dac.SQ, recs, bed)[0],
            "succinct": dac.expected_succinct(plain["succinct"], plain["complete"], dac.SQ, recs, bed),
            "only": dac.expected_complete(plain["complete"], dac.SQ, recs, bed, features_only=True)[0]}
    assert want["only"].count(b"\n") < want["complete"].count(b"\n") and b";" in want["complete"]
    return dict(dir=d, sam=d / "db.sam", bam=d / "db.bam", fa=d / "g.fa", bed=d / "f.bed", plain=plain, want=want)


KINDS = {"complete": ["--mode", "complete"], "succinct": ["--mode", "succinct"], "only": ["--mode", "complete", "--features-only"]}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sam_and_bam_host_and_gpu_routes(db, kind):
    base = ["decode"] + KINDS[kind] + ["--annotate", db["bed"]]
    want = db["want"][kind]
    r = run(base + [db["sam"], db["fa"]])
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
    host = run(base + ["--bgzf", "host", db["bam"], db["fa"]])
    gpu = run(base + ["--bgzf", "gpu", db["bam"], db["fa"]])
    assert host.returncode == 0 and gpu.returncode == 0, (host.stderr, gpu.stderr)
    assert host.stdout == gpu.stdout == want
    for extra, source, bgzf in ((["--batch-size", "1"], db["bam"], "gpu"), (["--batch-size", "3", "--fasta", "gpu"], db["sam"], "host"),
                                (["--batch-size", "3", "--fasta", "gpu"], db["bam"], "host")):
        r = run(base + extra + ["--bgzf", bgzf, source, db["fa"]])
        assert r.returncode == 0 and r.stdout == want, (extra, source, bgzf, r.stderr)
    out = db["dir"] / f"{kind}.csv"
    r = run(base + ["--bgzf", "gpu", "-o", out, db["bam"], db["fa"]])
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == want
    # without the option the bytes are what they were
    mode = KINDS[kind][1]
    assert run(["decode", "--mode", mode, "--bgzf", "gpu", db["bam"], db["fa"]]).stdout == db["plain"][mode]


def test_usage_errors_come_before_any_file_is_read(db):
    missing = db["dir"] / "missing"
    for args in (["decode", "--mode", "complete", "--features-only", missing, missing],
                 ["decode", "--mode", "succinct", "--annotate", missing, "--features-only", missing, missing],
                 ["decode", "--annotate", missing, "--features-only", missing, missing]):
        r = run(args, text=True)
        assert r.returncode == 2 and r.stderr.startswith("error: --features-only ") and "error: cannot read" not in r.stderr, r.stderr
        assert r.stdout == ""
    r = run(["decode", "--annotate"], text=True)
    assert r.returncode == 2


def test_a_malformed_bed_ends_like_enumerate_annotate(db, tmp_path):
    """exit status and message are those of `enumerate --annotate` on the same file against the same chromosomes"""
    fa = tmp_path / "g.fa"
    dac.write_fasta(fa, {n: s + "A" * (ln - len(s)) for (n, ln), s in zip(dac.SQ, dac.small_genome().values())})   # LN bases each
    prefix = tmp_path / "g"
    assert run(["index", "--index", prefix, fa]).returncode == 0
    kmers = tmp_path / "k.csv"
    kmers.write_text("id,sequence,pam,chromosome,position,sense\ng,ACGTTGCAAGCTTGCATGCA,NGG,cA,1,+\n")
    cases = {"order": ("cA\t0\t5\tok\ncA\t9\t4\tbad\n", db["sam"], []), "beyond": ("cB\t0\t65\n", db["bam"], ["--bgzf", "gpu"]),
             "few": ("# c\ncA\t0\t5\tok\n\ncA\t7\n", db["bam"], []), "semicolon": ("cA\t0\t5\tgene;exon\n", db["sam"], []),
             "empty": ("# nothing\n", db["bam"], ["--bgzf", "gpu"])}
    for name, (text, source, more) in cases.items():
        bed = tmp_path / f"{name}.bed"
        bed.write_text(text)
        out = tmp_path / f"{name}.csv"
        d = run(["decode", "--mode", "complete", "--annotate", bed, "-o", out] + more + [source, db["fa"]], text=True)
        e = run(["enumerate", prefix, "-f", kmers, "-m", 1, "--annotate", bed, "-o", tmp_path / "e.csv"], text=True)
        assert d.returncode == e.returncode == 1, (name, d.stderr, e.stderr)
        assert d.stderr == e.stderr and d.stderr.startswith("error: ") and len(d.stderr.splitlines()) == 1, (name, d.stderr, e.stderr)
        assert not out.exists() and d.stdout == ""
    r = run(["decode", "--annotate", tmp_path / "none.bed", db["sam"], db["fa"]], text=True)
    assert r.returncode == 1 and "cannot read the annotation file" in r.stderr
    # without -o nothing has been printed when the BED file is refused: it is read before the header line goes out
    r = run(["decode", "--annotate", tmp_path / "order.bed", db["sam"], db["fa"]], text=True)
    assert r.returncode == 1 and r.stdout == "" and "annotation line 2: start >= end" in r.stderr

"""`guidescan kmers` and `guidescan enumerate --all-candidates`: the kmers file of every candidate of an indexed genome,
and the database of those candidates, from one command each.

The kmers file must be the file the numpy restatement of the reference's script writes for the FASTA
(kmers.write_kmers_csv(device=None), pinned on the script's own rows by tests/test_kmers.py).  The database must be the
file `enumerate -f` writes for that kmers file - under the device encoder, where candidates, ids and senses never leave
HBM, and under the host encoders - and, once, the file the compiled reference (oracle/_ref/gs_ref_enumerate) writes.
GPU only."""
import io
import math
import os
import re
import subprocess
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
import test_oracle_vs_ref_pipeline as pipe

kmers = import_module("guidescan-cli_amd.kmers")

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
live = pipe.ref is not None and pipe.SHIM.exists()

# the option sets of tests/test_cli_encoder_gpu.py (a copy of its table, without the golden files: here the yardstick is
# the file `enumerate -f` writes)
RUNS = {
    "csv": ["-m", "3"],
    "sam": ["-m", "3", "--format", "sam"],
    "bam": ["-m", "3", "--format", "bam", "-n", "3"],
    "start": ["-m", "2", "--start"],
    "threshold": ["-m", "2", "-t", "1"],
    "succinct": ["-m", "3", "--mode", "succinct"],
    "sam_succinct": ["-m", "2", "--format", "sam", "--mode", "succinct"],
    "nag_max2": ["-m", "3", "-a", "NAG", "--max-off-targets", "2", "--format", "sam"],
}


def run(args, **kw):
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env, **kw)


def write_fasta(path, records, width=60):
    with open(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + name.encode() + b" seeded\n")
            for s in range(0, len(seq), width):
                f.write(seq[s:s + width] + b"\n")


def contig_records(n_contigs, seed, lo=150, hi=3000, odd=True):
    """seeded contigs of lo..hi bases; with `odd` a few shorter than k + P, one of N only, some in lower case, some with
    an N run"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_contigs):
        ln = int(rng.integers(lo, hi + 1))
        if odd and i % 50 == 7:
            ln = int(rng.integers(1, 23))  # shorter than k + P = 23: no candidate fits
        seq = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=ln).tobytes())
        if odd and i == 31:
            seq = bytearray(b"N" * ln)
        elif odd and i % 9 == 4 and ln > 100:
            a = int(rng.integers(0, ln - 40))
            seq[a:a + 30] = b"N" * 30
        if odd and i % 6 == 2:
            seq = bytearray(bytes(seq).lower())
        elif odd and i % 6 == 3:
            seq[ln // 3: ln // 2] = bytes(seq[ln // 3: ln // 2]).lower()
        out.append((f"ctg{i:03d}", bytes(seq)))
    return out


def expected_kmers(fasta, pam="NGG", k=20, start=False, prefix="", min_chr_length=0, chromosomes=None):
    buf = io.StringIO()
    recs = [(n, s) for n, s in kmers.fasta_records(fasta) if chromosomes is None or n in chromosomes]
    kmers.write_kmers_csv(buf, recs, pam, k, start, prefix, min_chr_length)
    return buf.getvalue().encode()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("allcand")


@pytest.fixture(scope="module")
def toy_index(toy, work):
    r = run(["index", "--index", work / "toy", toy["dir"] / "toy.fa"])
    assert r.returncode == 0, r.stderr
    return work / "toy"


@pytest.fixture(scope="module")
def contigs(work):
    """-> (FASTA, index prefix) of the 200-contig genome"""
    fa = work / "contigs.fa"
    write_fasta(fa, contig_records(200, seed=5))
    r = run(["index", "--index", work / "contigs", fa])
    assert r.returncode == 0, r.stderr
    return fa, work / "contigs"


KMERS_OPTIONS = {
    "default": ([], dict()),
    "tttn_start": (["--start", "--pam", "TTTN", "--kmer-length", "23"], dict(start=True, pam="TTTN", k=23)),
    "nag": (["--pam", "NAG"], dict(pam="NAG")),
    "min_chr_length": (["--min-chr-length", "1000"], dict(min_chr_length=1000)),
    "prefix": (["--prefix", "lib_"], dict(prefix="lib_")),
    "chromosomes": (["--chromosomes", "ctg012,ctg003"], dict(chromosomes=("ctg003", "ctg012"))),
}


@pytest.mark.parametrize("name", sorted(KMERS_OPTIONS))
def test_kmers_writes_the_scripts_file(toy, toy_index, contigs, work, name):
    opts, kw = KMERS_OPTIONS[name]
    fa, prefix = contigs
    cases = [(fa, prefix)] if name == "chromosomes" else [(fa, prefix), (toy["dir"] / "toy.fa", toy_index)]
    for fasta, px in cases:
        out = work / f"kmers_{name}_{px.name}.csv"
        r = run(["kmers", px, "-o", out] + opts)
        assert r.returncode == 0, r.stderr
        want = expected_kmers(fasta, **kw)
        assert out.read_bytes() == want
        assert want.count(b"\n") > 20 and not (work / (out.name + ".tmp")).exists()
        assert re.search(r"Wrote (\d+) candidate", r.stdout).group(1) == str(want.count(b"\n") - 1)


def kmers_file(prefix, work, start=False):
    out = work / f"{prefix.name}.kmers{'_start' if start else ''}.csv"
    if not out.exists():
        r = run(["kmers", prefix, "-o", out] + (["--start"] if start else []))
        assert r.returncode == 0, r.stderr
    return out


def three_files(prefix, work, name, opts, extra=()):
    """-> (enumerate -f <the kmers file>, --all-candidates under the host encoders, --all-candidates --encoder gpu, the
    last run's stdout)"""
    ext = "bam" if "bam" in opts else "sam" if "sam" in opts else "csv"
    opts = list(opts) + ([] if "-n" in opts else ["-n", "1"]) + list(extra)
    outs, log = [], ""
    for tag, source in (("f", ["-f", kmers_file(prefix, work, "--start" in opts)]), ("host", ["--all-candidates"]),
                        ("gpu", ["--all-candidates", "--encoder", "gpu"])):
        out = work / f"{prefix.name}_{name}.{tag}.{ext}"
        r = run(["enumerate", prefix, "-o", out] + source + opts)
        assert r.returncode == 0, (tag, r.stderr)
        outs.append(out.read_bytes())
        log = r.stdout
    return outs[0], outs[1], outs[2], log


def encoded(log):
    m = re.search(r"Encoder: gpu \((\d+) batch\(es\) encoded on the device, (\d+) by the host encoders\)", log)
    assert m, log
    return int(m.group(1)), int(m.group(2))


def candidates_line(log):
    m = re.search(r"Candidates: (\d+) guide\(s\) from (\d+) chromosome\(s\) in (\d+) batch\(es\)", log)
    assert m, log
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("name", sorted(RUNS))
def test_all_candidates_writes_the_file_of_the_kmers_file(toy_index, work, name):
    from_file, host, gpu, log = three_files(toy_index, work, name, RUNS[name])
    assert len(from_file) > 1000
    assert host == from_file
    assert gpu == from_file
    on_device, on_host = encoded(log)
    assert on_device >= 1 and on_host == 0
    n, n_chr, _ = candidates_line(log)
    assert n_chr == 3 and n == kmers_file(toy_index, work, "--start" in RUNS[name]).read_bytes().count(b"\n") - 1


def test_batches_cross_chromosome_boundaries(contigs, work):
    _, prefix = contigs
    from_file, host, gpu, log = three_files(prefix, work, "b4096", ["-m", "2"], extra=["--batch-size", "4096"])
    assert gpu == from_file and host == from_file
    n, n_chr, n_batches = candidates_line(log)
    assert n_chr == 200 and n > 3 * 4096
    assert n_batches <= math.ceil(n / 4096) + 1  # 200 chromosomes, far fewer batches: a batch holds several
    assert encoded(log) == (n_batches, 0)


def test_small_batches_in_bam(toy_index, work):
    """--batch-size 7 on the whole toy genome, BAM, four formatting threads"""
    from_file, host, gpu, log = three_files(toy_index, work, "bam7all", ["-m", "3", "--format", "bam", "-n", "4"],
                                            extra=["--batch-size", "7"])
    assert gpu == from_file and host == from_file
    assert encoded(log)[1] == 0


def test_a_shape_beyond_the_key_takes_the_host_route(toy_index, work):
    """L = 25, P = 4: 2L + 3P > 59, every batch answers GS_ERR_UNSUPPORTED and is copied to the host"""
    opts = ["--pam", "TTTN", "--kmer-length", "25", "--start", "-m", "1", "--chromosomes", "chrC", "-n", "1"]
    r = run(["kmers", toy_index, "-o", work / "k25.csv", "--pam", "TTTN", "--kmer-length", "25", "--start", "--chromosomes", "chrC"])
    assert r.returncode == 0, r.stderr
    r = run(["enumerate", toy_index, "-f", work / "k25.csv", "-o", work / "k25.f.csv", "--start", "-m", "1", "-n", "1"])
    assert r.returncode == 0, r.stderr
    r = run(["enumerate", toy_index, "--all-candidates", "--encoder", "gpu", "-o", work / "k25.gpu.csv"] + opts)
    assert r.returncode == 0, r.stderr
    assert (work / "k25.gpu.csv").read_bytes() == (work / "k25.f.csv").read_bytes()
    assert encoded(r.stdout)[0] == 0 and len((work / "k25.f.csv").read_bytes()) > 500


@pytest.mark.skipif(not live, reason="oracle/_ref not built")
@pytest.mark.parametrize("genome", ["toy", "four_contigs"])
def test_all_candidates_equals_the_compiled_reference(toy, work, genome):
    if genome == "toy":
        fa = toy["dir"] / "toy.fa"
    else:
        fa = work / "four.fa"
        write_fasta(fa, contig_records(4, seed=17, lo=4000, hi=9000, odd=False))
    prefix = work / f"ref_{genome}"
    r = run(["index", "--sdsl", "--index", prefix, fa])  # .forward / .reverse for the reference, .dna for the scan
    assert r.returncode == 0, r.stderr
    kcsv = work / f"ref_{genome}.kmers.csv"
    assert run(["kmers", prefix, "-o", kcsv]).returncode == 0
    want = pipe.run_shim(prefix, kcsv, work / f"ref_{genome}.want.csv", m=2, fmt="csv", complete=True)
    out = work / f"ref_{genome}.got.csv"
    r = run(["enumerate", prefix, "--all-candidates", "--encoder", "gpu", "-m", "2", "-o", out, "-n", "1"])
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == want and want.count(b"\n") > 1000
    assert encoded(r.stdout)[1] == 0


def test_errors_name_their_cause_and_leave_no_file(toy, toy_index, work):
    out = work / "never.csv"
    kcsv = kmers_file(toy_index, work)

    def refused(args, *words):
        r = run(args)
        assert r.returncode != 0 and not out.exists(), args
        for w in words:
            assert w in r.stderr, (w, r.stderr)

    refused(["enumerate", toy_index, "-f", kcsv, "--all-candidates", "-o", out], "-f", "--all-candidates", "exclude")
    refused(["enumerate", toy_index, "-o", out], "-f KMERS or --all-candidates")
    # a prefix with the reference's index files only
    sd = work / "sdsl_only"
    for ext in (".forward", ".reverse"):
        (work / ("sdsl_only" + ext)).write_bytes((toy["dir"] / ("toy.idx" + ext)).read_bytes())
    (work / "sdsl_only.gs").write_bytes((toy["dir"] / "toy.gs").read_bytes())
    refused(["enumerate", sd, "--all-candidates", "-o", out], "--all-candidates needs", "sdsl_only.dna", ".forward")
    # lengths that do not sum to the text's size
    bad = work / "bad_gs"
    (work / "bad_gs.dna").write_bytes((work / "toy.dna").read_bytes())
    (work / "bad_gs.gs").write_text((work / "toy.gs").read_text().replace("8000", "8001"))
    refused(["enumerate", bad, "--all-candidates", "-o", out], "bad_gs.gs sum to 58001", "58000")
    refused(["kmers", bad, "-o", out], "bad_gs.gs sum to 58001", "58000")
    refused(["enumerate", toy_index, "--all-candidates", "--chromosomes", "chrA,chrZ", "-o", out], "chrZ")
    refused(["kmers", toy_index, "--chromosomes", "chrZ", "-o", out], "chrZ")
    assert not (work / "never.csv.tmp").exists()

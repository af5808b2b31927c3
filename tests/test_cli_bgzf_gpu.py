"""`guidescan enumerate --format bam --bgzf gpu`: batches that are all fast path leave the device as BGZF members (records
and deflate made in HBM), any other batch takes the host's records and zlib.  The file holds the same records as the
`--bgzf host` file - only the deflate differs - reads back as the `--format sam` file, and decodes to the same CSV.
GPU only."""
import gzip
import re
import subprocess

import pytest

import bam_reader
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"


@pytest.fixture(scope="module")
def indexed(toy, tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf")
    subprocess.run([str(CLI), "index", "--index", str(d / "toy"), str(toy["dir"] / "toy.fa")], check=True, timeout=120)
    return d


def run(args, **kw):
    return subprocess.run([str(CLI)] + [str(a) for a in args], timeout=300, capture_output=True, text=True, **kw)


def on_device(log):
    m = re.search(r"encoder: bgzf gpu \((\d+) batch\(es\) compressed on the device, (\d+) by the host's zlib\)", log)
    assert m, log
    return int(m.group(1)), int(m.group(2))


def starred(sam_text):
    """a SAM file as a BAM reader prints it: the reference's empty RNAME comes back as '*'"""
    return "".join("\t".join(f if (i != 2 or f) else "*" for i, f in enumerate(l.split("\t"))) if not l.startswith("@") else l
                   for l in sam_text.splitlines(keepends=True))


def check(toy, indexed, name, source, opts, want_host_batches=0, gold=None):
    base = ["enumerate", indexed / "toy"] + source + ["-m", "3", "--mode", "complete"] + opts
    files = {}
    for tag, extra in (("host", ["--format", "bam"]), ("gpu", ["--format", "bam", "--bgzf", "gpu"]), ("sam", ["--format", "sam"])):
        files[tag] = indexed / f"{name}.{tag}"
        r = run(base + extra + ["-o", files[tag]], check=True)
        if tag == "gpu":
            dev, host = on_device(r.stdout)
            assert dev >= 1 and host == want_host_batches, r.stdout
        else:
            assert "bgzf gpu" not in r.stdout
    new, old = files["gpu"].read_bytes(), files["host"].read_bytes()
    sizes, eof = bam_reader.bgzf_blocks(new)
    assert eof and len(sizes) >= 3  # header block, members, the end-of-file block
    assert gzip.decompress(new) == gzip.decompress(old)
    sam = files["sam"].read_text()
    assert bam_reader.to_sam(files["gpu"]) == starred(sam) and len(sam) > 1000
    if gold:
        assert sam == (toy["dir"] / gold).read_text()
    fa = toy["dir"] / "toy.fa"
    csvs = [run(["decode", "--mode", "complete", files[tag], fa], check=True).stdout for tag in ("gpu", "host")]
    assert csvs[0] == csvs[1] and csvs[0].count("\n") > 10
    return new


@pytest.mark.parametrize("batch", [None, 7], ids=["default", "batch7"])
def test_kmers_file(toy, indexed, batch):
    opts = ["--batch-size", str(batch)] if batch else []
    check(toy, indexed, f"f{batch}", ["-f", toy["dir"] / "kmers.csv"], opts + ["-n", "3"], gold="ref_m3_sam.sam")


@pytest.mark.parametrize("batch", [None, 7], ids=["default", "batch7"])
def test_all_candidates(toy, indexed, batch):
    opts = ["--batch-size", str(batch)] if batch else []
    check(toy, indexed, f"all{batch}", ["--all-candidates", "--chromosomes", toy["names"][0]], opts + ["-n", "2"])


def test_a_batch_with_an_n_guide_takes_the_host_route(toy, indexed):
    lines = (toy["dir"] / "kmers.csv").read_text().splitlines()
    f = lines[1].split(",")
    f[0], f[1] = "withN", f[1][:7] + "N" + f[1][8:]
    kmers = indexed / "kmers_n.csv"
    kmers.write_text("\n".join(lines[:4] + [",".join(f)] + lines[4:]) + "\n")
    check(toy, indexed, "n", ["-f", kmers], ["--batch-size", "5", "-n", "2"], want_host_batches=1)


def test_bgzf_gpu_needs_format_bam(toy, indexed):
    for fmt in (["--format", "csv"], ["--format", "sam"], []):
        r = run(["enumerate", indexed / "toy", "-f", toy["dir"] / "kmers.csv", "-o", indexed / "no.out", "--bgzf", "gpu"] + fmt)
        assert r.returncode != 0 and "guidescan enumerate" in r.stderr and "--bgzf" in r.stderr
        assert not (indexed / "no.out").exists()
    r = run(["enumerate", indexed / "toy", "-f", toy["dir"] / "kmers.csv", "-o", indexed / "no.out", "--format", "bam", "--bgzf", "zstd"])
    assert r.returncode != 0

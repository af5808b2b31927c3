"""`guidescan index --fasta gpu` and `guidescan decode --fasta gpu`: the files and the table of the device FASTA reader are
byte for byte those of `--fasta host`, the messages for a record that occurs twice and for a file that cannot be read are
the host path's, and without --fasta nothing is different from before.  GPU only."""
import re
import subprocess

import pytest

import bam_make as bm
import decode_golden as dg
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"


def run(args, **kw):
    return subprocess.run([str(CLI)] + [str(a) for a in args], timeout=300, capture_output=True, **kw)


def index_inputs(toy):
    toy_fa = (toy["dir"] / "toy.fa").read_bytes()
    lines = toy_fa.split(b"\n")
    return {
        "toy": toy_fa,
        "crlf": b"\r\n".join(lines),
        # blanks at line ends: the .gs lengths count them, the .dna does not hold them (`guidescan kmers` documents it)
        "blanks_at_ends": b"\n".join((b"  " + ln + b" \t" if i % 7 == 3 and not ln.startswith(b">") else ln) for i, ln in enumerate(lines)),
        "ahead_of_title": b"acgtacgtnn\n  ACGT \n" + toy_fa,
        "no_newline_at_end": toy_fa.rstrip(b"\n"),
    }


@pytest.mark.parametrize("name", ["toy", "crlf", "blanks_at_ends", "ahead_of_title", "no_newline_at_end"])
def test_index_files_are_the_host_path_s(toy, tmp_path, name):
    fa = tmp_path / f"{name}.fa"
    fa.write_bytes(index_inputs(toy)[name])
    for how in ("host", "gpu"):
        r = run(["index", "--index", tmp_path / how, "--fasta", how, fa])
        assert r.returncode == 0, r.stderr
    assert (tmp_path / "gpu.gs").read_bytes() == (tmp_path / "host.gs").read_bytes()
    assert (tmp_path / "gpu.dna").read_bytes() == (tmp_path / "host.dna").read_bytes()
    assert (tmp_path / "gpu.dna").stat().st_size > 1000
    if name == "toy":   # the default is the host path, and the files are the fixture's
        assert run(["index", "--index", tmp_path / "dflt", fa]).returncode == 0
        assert (tmp_path / "dflt.gs").read_bytes() == (tmp_path / "host.gs").read_bytes() == (toy["dir"] / "toy.gs").read_bytes()
        assert (tmp_path / "dflt.dna").read_bytes() == (tmp_path / "host.dna").read_bytes()
        v = run(["index", "--index", tmp_path / "v", "--fasta", "gpu", "--verbose", fa])
        assert v.returncode == 0 and re.search(rb"Stages: FASTA read [0-9.]+ s, \.gs and \.dna writes [0-9.]+ s; fasta gpu: file reads", v.stderr)
        assert (tmp_path / "v.dna").read_bytes() == (tmp_path / "host.dna").read_bytes()
    if name == "blanks_at_ends":
        lengths = [int(x) for x in (tmp_path / "gpu.gs").read_text().split("\n")[1::2] if x]
        assert sum(lengths) > (tmp_path / "gpu.dna").stat().st_size


def test_index_errors(tmp_path):
    for how in ("host", "gpu"):
        r = run(["index", "--index", tmp_path / "x", "--fasta", how, tmp_path / "absent.fa"])
        assert r.returncode == 1 and r.stderr.decode().strip() == f"error: cannot read {tmp_path / 'absent.fa'}"
    assert run(["index", "--fasta", "tpu", tmp_path / "absent.fa"]).returncode == 2


@pytest.fixture(scope="module")
def bam_db(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta_gpu")
    h, recs = bm.from_sam(dg.paths("toy_ref_m3_sam")[0].read_text())
    (d / "toy.bam").write_bytes(b"".join(bm.members(h + b"".join(recs), piece=20000)) + bm.EOF_BLOCK)
    return d / "toy.bam"


@pytest.mark.parametrize("mode", dg.MODES)
@pytest.mark.parametrize("name", ["hand", "toy_ref_m3_sam"])
def test_decode_sam_database(name, mode):
    sam, fa = dg.paths(name)
    host = run(["decode", "--mode", mode, "--fasta", "host", sam, fa])
    assert host.returncode == 0 and host.stdout == dg.expected(name, mode)
    gpu = run(["decode", "--mode", mode, "--fasta", "gpu", "--verbose", sam, fa])
    assert gpu.returncode == 0, gpu.stderr
    assert gpu.stdout == host.stdout
    assert re.search(rb"FASTA read [0-9.]+ s", gpu.stderr)
    assert re.search(rb"fasta gpu: file reads [0-9.]+ s, waits for the uploads [0-9.]+ s, device stage [0-9.]+ s \(its five passes [0-9.]+ s\)", gpu.stderr)


@pytest.mark.parametrize("mode", dg.MODES)
def test_decode_bam_database(bam_db, mode):
    fa = dg.paths("toy_ref_m3_sam")[1]
    host = run(["decode", "--mode", mode, bam_db, fa])
    assert host.returncode == 0 and host.stdout == dg.expected("toy_ref_m3_sam", mode)
    for bgzf in ("host", "gpu"):
        gpu = run(["decode", "--mode", mode, "--fasta", "gpu", "--bgzf", bgzf, bam_db, fa])
        assert gpu.returncode == 0, gpu.stderr
        assert gpu.stdout == host.stdout, bgzf


def test_missing_record_fails_alike(tmp_path):
    sam = dg.paths("hand")[0]
    fa = dg.DIR / "hand_missing.fa"
    host = run(["decode", "--mode", "complete", "--fasta", "host", sam, fa])
    gpu = run(["decode", "--mode", "complete", "--fasta", "gpu", sam, fa])
    assert host.returncode == 1 and b"an off-target on a chromosome that the FASTA does not hold" in host.stderr
    assert host.stderr.startswith(b"error: gs_decode: record ")
    assert (gpu.returncode, gpu.stdout, gpu.stderr) == (host.returncode, host.stdout, host.stderr)


def test_record_twice_and_unreadable_file(tmp_path):
    sam, fa = dg.paths("hand")
    twice = tmp_path / "twice.fa"
    twice.write_bytes(fa.read_bytes() + b">extra\nACGT\n" + fa.read_bytes())
    out = {}
    for how in ("host", "gpu"):
        r = run(["decode", "--fasta", how, "-o", tmp_path / f"{how}.csv", sam, twice])
        assert r.returncode == 1 and r.stdout == b"" and not (tmp_path / f"{how}.csv").exists()
        out[how] = r.stderr
        r = run(["decode", "--fasta", how, sam, tmp_path / "absent.fa"])
        assert r.returncode == 1 and r.stderr.decode().strip() == f"error: cannot read {tmp_path / 'absent.fa'}"
    assert out["gpu"] == out["host"]
    assert re.fullmatch(rb"error: FASTA record '[^']+' occurs twice in \S+twice\.fa\n", out["host"])
    assert run(["decode", "--fasta", "tpu", sam, fa]).returncode == 2


def test_default_is_the_host_reader():
    sam, fa = dg.paths("hand")
    dflt = run(["decode", "--verbose", sam, fa])
    host = run(["decode", "--verbose", "--fasta", "host", sam, fa])
    assert dflt.returncode == 0 and dflt.stdout == host.stdout == dg.expected("hand", "succinct")
    shape = rb"Decoded \d+ records in [0-9.]+ s: FASTA read [0-9.]+ s, library calls \(decoder's batches, text back\) [0-9.]+ s, " \
            rb"output writes [0-9.]+ s, database read and decoder set-up [0-9.]+ s\n"
    assert re.fullmatch(shape, dflt.stderr) and re.fullmatch(shape, host.stderr)   # the stage line, and nothing else

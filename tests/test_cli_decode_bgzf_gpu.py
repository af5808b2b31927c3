"""`guidescan decode --bgzf gpu`: the table of a BAM database inflated, split and decoded on the device is byte for byte
the table of `--bgzf host` - in both modes, on BAM files built from the fixtures and on one our own
`enumerate --format bam --bgzf gpu` wrote, whatever --batch-size cuts the groups to; a damaged file ends with exit status
1, the documented message and no -o file; a SAM database with --bgzf gpu is a usage error.  GPU only."""
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


@pytest.fixture(scope="module")
def files(toy, tmp_path_factory):
    """name -> (BAM file, FASTA)"""
    d = tmp_path_factory.mktemp("decode_bgzf")
    out = {}
    sq, index, rows, sam = bm.hand_database()
    head = bm.header("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in sq), sq)
    raw = head + b"".join(bm.build(rows, index))
    (d / "hand_rows.bam").write_bytes(b"".join(bm.members(raw, piece=3000)) + bm.EOF_BLOCK)
    out["hand_rows"] = (d / "hand_rows.bam", dg.DIR / "hand.fa")
    h, recs = bm.from_sam(dg.paths("toy_ref_m3_sam")[0].read_text())
    (d / "toy_built.bam").write_bytes(b"".join(bm.members(h + b"".join(recs) * 3, piece=20000)) + bm.EOF_BLOCK)
    out["toy_built"] = (d / "toy_built.bam", dg.paths("toy_ref_m3_sam")[1])
    fa = toy["dir"] / "toy.fa"
    subprocess.run([str(CLI), "index", "--index", str(d / "toy"), str(fa)], check=True, timeout=120)
    subprocess.run([str(CLI), "enumerate", str(d / "toy"), "-f", str(toy["dir"] / "kmers.csv"), "-o", str(d / "ours.bam"), "-m", "3",
                    "--format", "bam", "--bgzf", "gpu"], check=True, timeout=300, capture_output=True)
    out["ours"] = (d / "ours.bam", fa)
    out["dir"] = d
    return out


@pytest.mark.parametrize("name", ["hand_rows", "toy_built", "ours"])
@pytest.mark.parametrize("mode", dg.MODES)
def test_gpu_route_equals_host_route(files, name, mode):
    bam, fa = files[name]
    host = run(["decode", "--mode", mode, "--bgzf", "host", bam, fa])
    assert host.returncode == 0 and host.stdout.count(b"\n") > 5
    assert run(["decode", "--mode", mode, bam, fa]).stdout == host.stdout   # host is the default
    for extra in ([], ["--batch-size", "1"], ["--batch-size", "7"]):
        gpu = run(["decode", "--mode", mode, "--bgzf", "gpu", "--verbose"] + extra + [bam, fa])
        assert gpu.returncode == 0, gpu.stderr
        assert gpu.stdout == host.stdout, extra
        m = re.search(rb"bgzf gpu: (\d+) members, (\d+) bytes inflated on the device", gpu.stderr)
        assert m and int(m.group(1)) >= 2 and int(m.group(2)) > 100
    if name == "ours":
        assert host.stdout == dg.expected("toy_ref_m3_sam", mode)
    out = files["dir"] / f"{name}.{mode}.csv"
    assert run(["decode", "--mode", mode, "--bgzf", "gpu", "-o", out, bam, fa]).returncode == 0
    assert out.read_bytes() == host.stdout


def test_damaged_files(files):
    bam, fa = files["toy_built"]
    d = files["dir"]
    data = bytearray(bam.read_bytes())
    sizes = dg.decode.bgzf_member_sizes(bytes(data))
    assert len(sizes) >= 4
    # a byte of the third member's deflate stream
    at = sizes[0] + sizes[1] + 18 + (sizes[2] - 26) // 2
    data[at] ^= 0x55
    (d / "flip.bam").write_bytes(bytes(data))
    r = run(["decode", "--bgzf", "gpu", "-o", d / "flip.csv", d / "flip.bam", fa], text=True)
    assert r.returncode == 1 and not (d / "flip.csv").exists()
    assert re.search(r"error: malformed BAM file \S+flip.bam: gs_bgzf_inflate: member 2 at byte %d: " % (sizes[0] + sizes[1]), r.stderr), r.stderr
    # with small groups the member is named within its group, and the rows before it are on stdout already (no -o)
    r = run(["decode", "--bgzf", "gpu", "--batch-size", "1", d / "flip.bam", fa], text=True)
    assert r.returncode == 1 and r.stdout.startswith("id,")
    assert "gs_bgzf_inflate: member 2 at byte %d: " % (sizes[0] + sizes[1]) in r.stderr, r.stderr
    # the file cut inside a member
    (d / "cut.bam").write_bytes(bam.read_bytes()[:sizes[0] + sizes[1] + 100])
    r = run(["decode", "--bgzf", "gpu", "-o", d / "cut.csv", d / "cut.bam", fa], text=True)
    assert r.returncode == 1 and "a BGZF block is cut" in r.stderr and not (d / "cut.csv").exists()
    # the file cut between members, inside a record: the host route's words
    (d / "short.bam").write_bytes(bam.read_bytes()[:sizes[0] + sizes[1]])
    r = run(["decode", "--bgzf", "gpu", "-o", d / "short.csv", d / "short.bam", fa], text=True)
    h = run(["decode", "--bgzf", "host", d / "short.bam", fa], text=True)
    assert r.returncode == 1 and h.returncode == 1 and "a record is cut" in r.stderr and "a record is cut" in h.stderr
    assert not (d / "short.csv").exists()


def test_sam_database_with_bgzf_gpu_is_a_usage_error(files):
    sam, fa = dg.paths("toy_ref_m3_sam")
    r = run(["decode", "--bgzf", "gpu", sam, fa], text=True)
    assert r.returncode == 2 and "usage:" in r.stderr and "--bgzf host|gpu" in r.stderr
    assert run(["decode", "--bgzf", "host", sam, fa]).returncode == 0
    assert run(["decode", "--bgzf", "both", files["toy_built"][0], fa]).returncode == 2

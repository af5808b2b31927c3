"""GenomeIndex.save_sdsl / `guidescan index --sdsl`: the reference's own index files written from the GPU-built index
(gs_sdsl_export.hip), byte for byte.

 * the toy genome against tests/golden/toy/toy.idx.forward / .reverse (written by the reference's own `index` command),
   from a built handle, from one opened with open_sdsl and from one opened with open_sa, and through the CLI;
 * a 12 Mbp genome with N runs: the exported prefix, opened again with open_sdsl, answers a batch as the built handle does;
 * where oracle/_ref is built: whole files against the compiled reference containers' writer, fed this index's own suffix
   arrays (proved first from the text alone), at chr1 size - where the compiled reference then also enumerates from OUR
   files - for a 20 kbp genome (select_support_mcl's init_slow side) and for a genome with a 1 Mbp run of one base
   (a select superblock stored long).  Nothing reads the reference tree.  GPU only."""
import os
import subprocess
import threading
import time
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
from sdsl_walk import walk

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
SHIM = ol.ORACLE_DIR / "_ref" / "gs_ref_enumerate"
NGG = np.frombuffer(b"NGG", np.uint8)
GS_ERR_ARG = 1

ref = ol.ref()
needs_ref = pytest.mark.skipif(ref is None or not SHIM.exists(), reason="oracle/_ref not built (no reference tree)")


def golden(toy, strand):
    return (toy["dir"] / f"toy.idx.{strand}").read_bytes()


def assert_files_equal(got, want, what):
    """whole files, and on a difference the first section of the App. A walk that differs"""
    a, b = open(got, "rb").read(), open(want, "rb").read()
    if a == b:
        return
    sec, _ = walk(b)
    first = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    where = [k for k, (s, e) in sec.items() if s <= first < e]
    raise AssertionError(f"{what}: {len(a)} bytes against the reference's {len(b)}, first difference at byte {first} "
                         f"(section {where})")


def test_toy_export_equals_the_reference_index_command(toy, tmp_path):
    gidx = api.GenomeIndex.build(toy["text"], device=0)
    try:
        gidx.save_sdsl(toy["text"], tmp_path / "t")
    finally:
        gidx.close()
    assert (tmp_path / "t.forward").read_bytes() == golden(toy, "forward")
    assert (tmp_path / "t.reverse").read_bytes() == golden(toy, "reverse")
    assert sorted(os.listdir(tmp_path)) == ["t.forward", "t.reverse"]   # no temporary file stays


def test_toy_export_from_an_imported_handle(toy, tmp_path):
    gidx = api.GenomeIndex.open_sdsl(toy["dir"] / "toy.idx", device=0)
    try:
        gidx.save_sdsl(toy["text"], tmp_path / "t")
    finally:
        gidx.close()
    assert (tmp_path / "t.forward").read_bytes() == golden(toy, "forward")
    assert (tmp_path / "t.reverse").read_bytes() == golden(toy, "reverse")


def test_toy_export_from_a_stored_suffix_array_handle(toy, tmp_path):
    gidx = api.GenomeIndex.build(toy["text"], device=0)
    try:
        gidx.save_sa(toy["text"], tmp_path / "t.sa")
    finally:
        gidx.close()
    gidx = api.GenomeIndex.open_sa(toy["text"], tmp_path / "t.sa", device=0)
    try:
        gidx.save_sdsl(toy["text"], tmp_path / "t")
    finally:
        gidx.close()
    assert (tmp_path / "t.forward").read_bytes() == golden(toy, "forward")
    assert (tmp_path / "t.reverse").read_bytes() == golden(toy, "reverse")


def test_round_trip_12mbp_with_n_runs(tmp_path):
    text, names, lengths = synth.make_genome([7_000_000, 5_000_000], seed=21)
    assert (text == ord("N")).any()
    seqs, pams, pos, strands = synth.sample_guides(text, 2000, seed=22)
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        off, hits, _ = gidx.enumerate(seqs, pams, mismatches=3)
        gidx.save_sdsl(text, tmp_path / "g")
        off2, hits2, _ = gidx.enumerate(seqs, pams, mismatches=3)
        assert np.array_equal(off, off2) and hits.tobytes() == hits2.tobytes()   # the handle is as it was
        again = api.GenomeIndex.open_sdsl(tmp_path / "g", device=0)
        try:
            off3, hits3, _ = again.enumerate(seqs, pams, mismatches=3)
        finally:
            again.close()
        assert np.array_equal(off, off3) and hits.tobytes() == hits3.tobytes()
        assert int(off[-1]) >= 2000
    finally:
        gidx.close()


# ---- against the compiled reference containers ----------------------------------------------------------------------

def proved_index(text):
    """the index, its suffix arrays proved from the text alone: a wrong file is never blamed on a wrong sort"""
    gidx = api.GenomeIndex.build(text, device=0)
    for s in (0, 1):
        rep = gidx.verify_sa(text, strand=s, samples="all")
        assert rep["rows"] == text.shape[0] + 1, rep
        assert rep["not_permutation"] == rep["out_of_order"] == rep["undecided"] == rep["bwt_mismatch"] == 0, rep
    return gidx


def reference_files(gidx, text, d):
    """<d>/ref.forward / .reverse through the compiled reference containers from this index's suffix arrays, a host
    thread per strand (ctypes releases the GIL)"""
    err = []

    def one(strand, suffix):
        try:
            n = text.shape[0] + 1
            sa = gidx.suffix_array(strand)
            st = np.ascontiguousarray(text if strand == 0 else synth.reverse_complement_bytes(text))
            h = ref.ref_index_build_text(st.ctypes.data, sa.ctypes.data, n, os.path.join(d, f"tmp{strand}.sdsl").encode())
            assert ref.ref_write_index_file(h, os.path.join(d, "ref" + suffix).encode()) == 0
            ref.ref_index_free(h)
        except Exception as e:
            err.append(repr(e))

    th = [threading.Thread(target=one, args=a) for a in ((0, ".forward"), (1, ".reverse"))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    return os.path.join(d, "ref")


def export_and_compare(text, d, what):
    gidx = proved_index(text)
    try:
        gidx.save_sdsl(text, os.path.join(d, "ours"))
        ref_prefix = reference_files(gidx, text, d)
        for suffix in (".forward", ".reverse"):
            assert_files_equal(os.path.join(d, "ours" + suffix), ref_prefix + suffix, what + suffix)
    except BaseException:
        gidx.close()
        raise
    return gidx, ref_prefix


@needs_ref
def test_small_genome_takes_the_init_slow_side(tmp_path):
    """20 kbp: m_bv is under 100,000 bits, so both select supports go through init_slow (select_support_mcl.hpp:108-116)"""
    text, _, _ = synth.make_genome([12_000, 8_000], seed=31)
    gidx, ref_prefix = export_and_compare(text, str(tmp_path), "20 kbp")
    gidx.close()
    bits = int.from_bytes(open(ref_prefix + ".forward", "rb").read()[16:24], "little")
    assert 0 < bits < 100_000, bits


@needs_ref
def test_genome_with_a_long_select_superblock(tmp_path):
    """a 1 Mbp run of one base in a random 3 Mbp text: its BWT run leaves far fewer than 4,096 set (or unset) bits in
    more than logn4 = 23^4 bits of the root node, so a superblock is stored long (select_support_mcl.hpp:303-319) - seen
    in the reference-written file itself, and not the last superblock (init_fast always stores an incomplete last one
    long, :332-342)"""
    rng = np.random.default_rng(5)
    text = rng.choice(np.frombuffer(b"ACGT", np.uint8), 3_000_000)
    text[1_000_000:2_000_000] = ord("A")
    gidx, ref_prefix = export_and_compare(text, str(tmp_path), "3 Mbp with a run")
    gidx.close()
    inner_long = 0
    for suffix in (".forward", ".reverse"):
        _, longs = walk(open(ref_prefix + suffix, "rb").read())
        inner_long += sum(1 for sb, idx in longs.values() for i in idx if i < sb - 1)
    assert inner_long >= 1, "the case no longer covers a long superblock: lengthen the run"


@needs_ref
def test_chr1_sized_files_and_the_reference_enumerating_from_them(tmp_path):
    """249 Mbp: both files byte for byte; then oracle/_ref/gs_ref_enumerate opens OUR files and its CSV data lines for 256
    guides at <= 3 mismatches equal the product's"""
    t0 = time.time()
    d = str(tmp_path)
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    gidx, ref_prefix = export_and_compare(text, d, "chr1-sized")
    try:
        for suffix in (".forward", ".reverse"):
            os.unlink(ref_prefix + suffix)
        with open(os.path.join(d, "ours.gs"), "w") as f:
            f.write("".join(f"{a}\n{b}\n" for a, b in zip(names, lengths)))
        n, m = 256, 3
        seqs, pams, pos, strands = synth.sample_guides(text, n, seed=41)
        ids = [f"g{i}" for i in range(n)]
        kcsv, out = os.path.join(d, "k.csv"), os.path.join(d, "o.csv")
        synth.write_kmers_csv(kcsv, ids, [s.tobytes().decode() for s in seqs], ["NGG"] * n, [names[0]] * n, [1] * n, ["+"] * n)
        env = dict(os.environ, GS_REF_THREADS="16")
        subprocess.run([str(SHIM), os.path.join(d, "ours"), kcsv, out, "csv", "complete", str(m), "0", "0", "-1", "-1", "0"],
                       env=env, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(out) as f:
            ref_lines = sorted(f.read().splitlines()[1:])
        gs = api.make_genome_structure(names, lengths)
        off, hits, _ = gidx.enumerate(seqs, np.tile(NGG, (n, 1)), mismatches=m)
        _, spec = gidx.score(gs, seqs, 3, off, hits, want_cfd=False)
        ours = []
        for i in range(n):
            ours += api.format_guide(gs, ids[i], seqs[i].tobytes().decode(), "NGG", True, hits[off[i]:off[i + 1]], m,
                                     specificity=spec[i]).splitlines()
        assert len(ref_lines) >= n and sorted(ours) == ref_lines
    finally:
        gidx.close()
    print(f"[sdsl export] chr1-sized case: {time.time() - t0:.1f} s")


# ---- command line ----------------------------------------------------------------------------------------------------

def test_cli_index_sdsl(toy, tmp_path):
    fa = str(toy["dir"] / "toy.fa")
    plain = tmp_path / "plain"
    plain.mkdir()
    subprocess.run([str(CLI), "index", "--index", str(plain / "toy"), fa], check=True, timeout=120)
    assert sorted(os.listdir(plain)) == ["toy.dna", "toy.gs"]   # without the flag: what it always wrote
    d = tmp_path / "sdsl"
    d.mkdir()
    r = subprocess.run([str(CLI), "index", "--sdsl", "--index", str(d / "toy"), fa], check=True, timeout=120,
                       capture_output=True, text=True)
    assert f"Wrote {d / 'toy'}.forward and {d / 'toy'}.reverse" in r.stdout
    assert sorted(os.listdir(d)) == ["toy.dna", "toy.forward", "toy.gs", "toy.reverse"]
    assert (d / "toy.forward").read_bytes() == golden(toy, "forward")
    assert (d / "toy.reverse").read_bytes() == golden(toy, "reverse")
    assert (d / "toy.dna").read_bytes() == (plain / "toy.dna").read_bytes()
    run = [str(CLI), "enumerate", str(d / "toy"), "-f", str(toy["dir"] / "kmers.csv"), "-m", "3", "-n", "1", "-o"]
    subprocess.run(run + [str(d / "with_dna.csv")], check=True, timeout=300)
    os.unlink(d / "toy.dna")
    subprocess.run(run + [str(d / "without_dna.csv")], check=True, timeout=300)   # opens through the importer
    assert (d / "without_dna.csv").read_bytes() == (d / "with_dna.csv").read_bytes()
    assert (d / "with_dna.csv").read_bytes() == (toy["dir"] / "ref_m3_csv.csv").read_bytes()


# ---- errors ----------------------------------------------------------------------------------------------------------

def test_errors_leave_no_file_and_a_usable_handle(toy, tmp_path):
    text = toy["text"]
    seqs, pams, pos, strands = synth.sample_guides(text, 32, seed=5)
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        off, hits, _ = gidx.enumerate(seqs, pams, mismatches=2)
        with pytest.raises(api.GsError) as e:
            gidx.save_sdsl(text[:-1], tmp_path / "short")
        assert e.value.status == GS_ERR_ARG
        assert os.listdir(tmp_path) == []
        missing = tmp_path / "no_such_directory"
        with pytest.raises(api.GsError) as e:
            gidx.save_sdsl(text, missing / "t")
        assert e.value.status != 0
        ro = tmp_path / "read_only"
        ro.mkdir()
        os.chmod(ro, 0o555)
        try:
            if not os.access(ro, os.W_OK):   # (a privileged user writes anywhere: the missing directory above stands in)
                with pytest.raises(api.GsError):
                    gidx.save_sdsl(text, ro / "t")
                assert os.listdir(ro) == []
        finally:
            os.chmod(ro, 0o755)
        assert sorted(os.listdir(tmp_path)) == ["read_only"]
        off2, hits2, _ = gidx.enumerate(seqs, pams, mismatches=2)
        assert np.array_equal(off, off2) and hits.tobytes() == hits2.tobytes()
        gidx.save_sdsl(text, tmp_path / "t")   # and exports
        assert (tmp_path / "t.forward").read_bytes() == golden(toy, "forward")
    finally:
        gidx.close()

"""The FASTA reader on the device (gs_fasta_parse, gs_fasta_parse_device, gs_fasta_parse_file, gs_decoder_open_fasta)
against the models of tests/fasta_model.py: the tile-edge files made for the device's tile size, random files of up to
eight tiles, a file read in several staging chunks, a CRLF genome, a raw buffer beyond 2^32 bytes, and the decoder opened
from the parsed object against the decoder opened from the host reader's records.  GPU only."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import decode_golden as dg
import fasta_model as fm

pytestmark = pytest.mark.gpu
api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")
seqio = import_module("guidescan-cli_amd.seqio")
decode = import_module("guidescan-cli_amd.decode")


def device_bytes(ptr, n):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.empty(n, dtype=np.uint8)
    assert hip.hipMemcpy(host.ctypes.data, ptr, n, 2) == 0
    return host.tobytes()


def check_file(raw, tmp_path, what, torch=None):
    """through gs_fasta_parse, and with torch also through gs_fasta_parse_device"""
    exp = fm.expected(raw, tmp_path)
    for rules in ("index", "records"):
        def parse_host():
            return api.DeviceFasta.parse(raw, rules)

        def parse_dev():
            buf = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda() if raw else torch.zeros(0, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            return api.DeviceFasta.parse_device(buf.data_ptr() if raw else None, len(raw), rules)

        for parse in (parse_host,) + ((parse_dev,) if torch is not None else ()):
            where = f"{what}, {rules} rules, {parse.__name__}: {raw[:60]!r}"
            if isinstance(exp[rules], fm.DuplicateRecord):
                with pytest.raises(api.GsError) as e:
                    parse()
                assert e.value.status == 6, where
                assert f"FASTA record '{exp[rules].name.decode('latin-1')}' occurs twice" in str(e.value), where
                continue
            with parse() as fa:
                fm.compare(api._fasta_result(fa), fa.records(), exp[rules], rules, where)


def test_tile_edge_files(tmp_path):
    torch = pytest.importorskip("torch")
    T = api.fasta_tile_bytes()
    for made_for in (T, 16):     # the tile, and the sixteen bytes of a lane: the same carries one level down
        for name, raw in fm.tile_edge_files(made_for).items():
            check_file(raw, tmp_path, f"{name} (made for {made_for})", torch)


def test_random_files(tmp_path):
    torch = pytest.importorskip("torch")
    T = api.fasta_tile_bytes()
    n = 0
    for raw in fm.random_files(100, 8 * T, seed=77, long_lines=True):
        check_file(raw, tmp_path, f"long-line file {n}", torch if n % 4 == 0 else None)
        n += 1
    for raw in fm.random_files(100, 8 * T, seed=78):
        check_file(raw, tmp_path, f"short-line file {n}", torch if n % 4 == 0 else None)
        n += 1
    assert n == 200


def test_unaligned_device_buffer(tmp_path):
    """raw bytes that do not begin on a 16-byte boundary take the byte loads"""
    torch = pytest.importorskip("torch")
    raw = next(iter(fm.random_files(1, 3 * api.fasta_tile_bytes(), seed=5, long_lines=True)))
    raw = b">first title\n" + raw
    exp = fm.expected(raw, tmp_path)["index"]
    buf = torch.frombuffer(bytearray(b"xxx" + raw), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with api.DeviceFasta.parse_device(buf.data_ptr() + 3, len(raw), "index") as fa:
        fm.compare(api._fasta_result(fa), fa.records(), exp, "index")


def test_file_in_several_chunks(tmp_path):
    chunk = 1 << 16
    before = api.fasta_chunk_bytes()
    raw = b"".join(b">r%d some words\r\n" % i + bytes(fm.random.Random(i).choices(b"acgtnACGTN \r\n", k=9000)) + b"\n" for i in range(16))
    raw = raw[:2 * chunk + 1] if len(raw) > 2 * chunk + 1 else raw
    assert len(raw) == 2 * chunk + 1           # two chunks and one byte
    p = tmp_path / "chunks.fa"
    p.write_bytes(raw)
    exp = fm.expected(raw, tmp_path)
    try:
        assert api.fasta_chunk_bytes(chunk) == chunk
        for rules in ("index", "records"):
            with api.DeviceFasta.parse(p, rules) as fa:
                fm.compare(api._fasta_result(fa), fa.records(), exp[rules], rules)
                assert set(fa.ms()) == {"read", "upload", "kernels", "names", "passes"}
    finally:
        api.fasta_chunk_bytes(before)
    with pytest.raises(api.GsError) as e:
        api.DeviceFasta.parse(tmp_path / "absent.fa", "index")
    assert e.value.status == 5 and "cannot read" in str(e.value)


def test_crlf_genome_equals_seqio(tmp_path):
    text, names, lengths = synth.make_genome([30_011, 12_345, 61], seed=9)
    blob, at = [], 0
    for n, ln in zip(names, lengths):
        blob.append(f">{n} made up\r\n".encode())
        chrom = text[at:at + ln].tobytes().lower()
        blob += [chrom[i:i + 60] + b"\r\n" for i in range(0, ln, 60)]
        at += ln
    p = tmp_path / "crlf.fa"
    p.write_bytes(b"".join(blob))
    want = seqio.parse_fasta(p)
    got = api.parse_fasta_device(p)
    assert got[0].tobytes() == want[0].tobytes() and got[0].tobytes() == text.tobytes().upper()
    assert got[1] == want[1] == names and got[2] == want[2]
    assert got[2] != lengths                   # the '\r' counts (seq_io.cxx:100-104)
    recs = api.parse_fasta_device(p.read_bytes(), rules="records")
    assert list(recs) == names and b"".join(recs.values()) == text.tobytes().lower()


def test_offsets_beyond_32_bits():
    """2^32 + 2^20 raw bytes made on the device: 60 x 'a' and a newline, over and over, with three title lines written
    over line starts, the last one beyond 2^32.  Everything expected follows from arithmetic."""
    torch = pytest.importorskip("torch")
    N = (1 << 32) + (1 << 20)
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * (1 << 30):
        pytest.skip(f"needs 12 GB of free device memory, {free >> 30} GB are free")
    period = torch.tensor(list(b"a" * 60 + b"\n"), dtype=torch.uint8, device="cuda")
    buf = period.repeat((N + 60) // 61)[:N]
    title_at = [0, 61 * 1000, 61 * (((1 << 32) + 5 + 60) // 61)]
    assert title_at[2] > (1 << 32) and title_at[2] + 61 < N
    for i, o in enumerate(title_at):
        buf[o:o + 4] = torch.tensor(list(b">c%d\n" % i), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    # the newlines in front of x are the periodic ones, x // 61 of them, and the titles' own (each where an 'a' stood)
    def kept_before(x):          # x is a line start: every byte in front that is no newline and no title byte
        nl = x // 61 + sum(1 for o in title_at if o < x)
        return x - nl - 3 * sum(1 for o in title_at if o < x)

    total_nl = N // 61 + 3
    total_kept = N - total_nl - 9
    ends = title_at[1:] + [N]
    with api.DeviceFasta.parse_device(buf.data_ptr(), N, "index") as fa:
        n, tl, _ = fa.info()
        assert (n, tl) == (3, total_kept)
        rec = fa.records()
        assert rec["names"] == [b"c0", b"c1", b"c2"]
        for i, o in enumerate(title_at):
            body = (o + 4, ends[i])                                   # raw bytes behind the title line
            nl = ends[i] // 61 - (o + 4) // 61                        # the periodic newlines among them
            assert int(rec["title_off"][i]) == o and int(rec["title_len"][i]) == 3
            assert int(rec["text_off"][i]) == kept_before(o), i
            assert int(rec["text_len"][i]) == body[1] - body[0] - nl, i
            assert int(rec["line_len"][i]) == body[1] - body[0] - nl, i   # no blanks: untrimmed = trimmed
        assert int(rec["text_off"][2]) + int(rec["text_len"][2]) == total_kept
        ptr = fa.text_device_ptr()
        around = kept_before(61 * ((1 << 32) // 61))                  # the text byte of a raw byte right below 2^32
        for at in [0, 1, around - 4097, around - 61, around - 1, around, around + 1, around + 60, around + 4096,
                   int(rec["text_off"][2]) - 1, int(rec["text_off"][2]), total_kept - 1]:
            assert device_bytes(ptr + at, 1) == b"A", at
    del buf


@pytest.mark.parametrize("name", sorted({n for n, m in dg.GOOD if m == "complete"}))
def test_decoder_opened_from_the_parsed_object(name):
    sam, fa = dg.paths(name)
    host = decode.decode_database(sam, fa, mode="complete", device=0)
    assert host.encode() == dg.expected(name, "complete")
    assert decode.decode_database(sam, fa, mode="complete", device=0, fasta="gpu") == host


def test_decode_database_checks_its_fasta_argument():
    sam, fa = dg.paths("hand")
    with pytest.raises(ValueError):
        decode.decode_database(sam, fa, device=0, fasta="tpu")
    with pytest.raises(ValueError):
        decode.decode_database(sam, fa, device=None, fasta="gpu")     # the model has no device to parse on


def test_decoder_open_fasta_missing_record_and_arguments():
    sam, _ = dg.paths("hand")
    sq, recs = decode.parse_sam(sam.read_text())
    missing = dg.DIR / "hand_missing.fa"
    with api.DeviceFasta.parse(missing, "records") as fa:
        with api.Decoder(sq, fa) as dec:       # a name without a record opens; its off-targets fail as on the host path
            with pytest.raises(api.GsError) as e1:
                dec.decode_records(recs, complete=True)
    with api.Decoder(sq, decode.parse_fasta_records(missing)) as dec:
        with pytest.raises(api.GsError) as e2:
            dec.decode_records(recs, complete=True)
    assert str(e1.value) == str(e2.value)
    with api.DeviceFasta.parse(missing, "index") as fa:
        with pytest.raises(api.GsError) as e:
            api.Decoder(sq, fa)
        assert e.value.status == 1              # an index-rules object is refused

"""The kmers-file reader on the device (gs_kmers_parse, gs_kmers_parse_device, gs_kmers_parse_file) against the
pure-Python model of the command's host reader (tests/kmers_file_model.py): the model's files made for the device's tile
and for its 16-byte window, lines of about a tile, an unaligned raw pointer, a file read in several staging chunks, the
round trip through the candidate scan's own rows, a concatenation of parsed parts, a raw buffer beyond 2^32 bytes, and the
database text from the parsed arrays against the text from the same rows passed from the host.  GPU only."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import kmers_file_model as km

pytestmark = pytest.mark.gpu
api = import_module("guidescan-cli_amd.api")


def device_array(ptr, n, dtype=np.uint8):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.empty(n, dtype=dtype)
    if n:
        assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0
    return host


def check_file(raw, what, torch=None, shift=0):
    """through gs_kmers_parse, and with torch also through gs_kmers_parse_device (the bytes `shift` past an aligned address)"""
    def parse_host():
        return api.DeviceKmers.parse(raw)

    def parse_dev():
        buf = torch.frombuffer(bytearray(b"x" * shift + raw + b"x"), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        return api.DeviceKmers.parse_device(buf.data_ptr() + shift, len(raw))

    for parse in (parse_host,) + ((parse_dev,) if torch is not None else ()):
        where = f"{what}, {parse.__name__}: {raw[:80]!r}"
        try:
            exp = km.parse(raw)
        except km.KmersError as e:
            with pytest.raises(api.KmersFileError) as got:
                parse()
            g = got.value
            assert (g.status, g.kind, g.message, g.text) == (6, e.kind, e.message, e.text), where
            if e.kind in (km.FEW, km.POSITION):
                assert (g.line, g.row) == (e.line, e.row), where
                assert raw[g.offset:g.offset + len(g.text)] == g.text, where
            continue
        if exp.mixed:
            with pytest.raises(api.GsError) as got:
                parse()
            assert got.value.status == 3, where
            continue
        parsed = parse()
        try:
            km.compare(api.kmers_arrays(parsed), exp, where)
            assert parsed.pos_ptr is None and parsed.to_host()[2] is None, where
            assert parsed.report["n_lines"] == len(km.lines_of(raw)), where
        finally:
            parsed.close()


def test_the_models_files():
    torch = pytest.importorskip("torch")
    T = api.kmers_tile_bytes()
    for made_for in (T, 16):     # the tile, and the sixteen bytes of a window
        files = km.good_files(made_for)
        assert "lines of about a tile" in files or made_for == 16
        for name, raw in files.items():
            check_file(raw, f"{name} (made for {made_for})", torch, shift=5 if made_for == 16 else 0)
    for name, (raw, _) in km.bad_files().items():
        check_file(raw, name, torch)
    for name, raw in km.mixed_files().items():
        check_file(raw, name, torch)


def test_golden_files():
    import oracle_lib as ol
    for name in ("toy", "config1"):
        raw = (ol.ROOT / "tests" / "golden" / name / "kmers.csv").read_bytes()
        check_file(raw, name)
        check_file(raw.replace(b"\n", b"\r\n"), name + " with CRLF")


def test_random_files():
    torch = pytest.importorskip("torch")
    n = 0
    for raw in km.random_files(150, seed=4242):
        check_file(raw, f"random file {n}", torch if n % 3 == 0 else None, shift=n % 16)
        n += 1


def test_lines_of_about_a_tile_over_three_tiles():
    T = api.kmers_tile_bytes()
    tail = b",ACGTACGTAC,NGG,chr2,77,-\r\n"
    for n in (T - 1, T, T + 1):
        raw = km.HEADER + b"".join(bytes([65 + i]) * (n - len(tail)) + tail for i in range(3))
        assert len(raw) > 3 * T - 3
        check_file(raw, f"three lines of {n} bytes")


def test_unaligned_device_pointer():
    torch = pytest.importorskip("torch")
    raw = km.HEADER + b"".join(km.row(i, sense=b"-+"[i % 2:][:1]) for i in range(700))      # several tiles
    assert len(raw) > 4 * api.kmers_tile_bytes()
    for shift in (1, 7, 15):
        check_file(raw, f"shifted by {shift}", torch, shift=shift)


def test_file_in_several_chunks(tmp_path):
    chunk = 1 << 16
    raw, i = km.HEADER, 0
    while len(raw) < 2 * chunk - 200:
        raw, i = raw + km.row(i), i + 1
    raw += b"last,ACGTACGTACGTACGTACGT,NGG,c,1,+"
    raw += b" " * (2 * chunk + 1 - len(raw))   # two chunks and one byte; the last line has no newline
    assert len(raw) == 2 * chunk + 1 and len(km.parse(raw).rows) == i + 1
    p = tmp_path / "chunks.csv"
    p.write_bytes(raw)
    before = api.kmers_chunk_bytes()
    try:
        assert api.kmers_chunk_bytes(chunk) == chunk
        parsed = api.DeviceKmers.parse(p)
        km.compare(api.kmers_arrays(parsed), km.parse(raw), "a file in three chunks")
        assert set(parsed.report["ms"]) >= {"file_reads", "upload_waits", "device_stage"} and parsed.report["ms"]["device_stage"] > 0
        parsed.close()
    finally:
        api.kmers_chunk_bytes(before)
    with pytest.raises(api.GsError) as e:
        api.DeviceKmers.parse(tmp_path / "absent.csv")
    assert e.value.status == 5 and "cannot read" in str(e.value)


def test_round_trip_through_the_scan(toy):
    """generate_kmers with encode_ids on the toy chromosomes, then the header plus csv() parsed: the scanned object's arrays"""
    parts, scanned, at = [], [], 0
    for name, ln in zip(toy["names"], toy["lengths"]):
        sc = api.generate_kmers(toy["text"][at:at + ln].tobytes(), "NGG", 20)
        at += ln
        sc.encode_ids("pre_", name)
        parsed = api.DeviceKmers.parse(km.HEADER + sc.csv("pre_", name))
        assert parsed.n == sc.n > 100
        seqs, pams, _, senses = sc.to_host()
        ids, off, sp = sc.ids_to_host()
        got = api.kmers_arrays(parsed)
        assert got["seqs"] == seqs.tobytes() and got["pams"] == pams.tobytes() and got["ids"] == ids
        assert np.array_equal(got["id_off"], off) and np.array_equal(got["sense"], sp)
        assert np.array_equal(parsed.to_host()[3], senses)                  # '+' / '-'
        for call in (lambda: parsed.encode_ids("", name), lambda: parsed.csv("", name)):
            with pytest.raises(api.GsError) as e:
                call()
            assert e.value.status == 1
        parts.append(parsed)
        scanned.append(sc)
    # concat_kmers of the parsed parts: the concatenation of the scanned ones
    both, want = api.concat_kmers(parts), api.concat_kmers(scanned)
    assert both.n == want.n == sum(p.n for p in parts) and both.pos_ptr is None
    a, b = both.to_host(), want.to_host()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] is None and np.array_equal(a[3], b[3])
    a, b = both.ids_to_host(), want.ids_to_host()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    with pytest.raises(api.GsError):
        api.concat_kmers([parts[0], scanned[0]])                            # rows of a file and candidates of a scan
    for k in parts + scanned + [both, want]:
        k.close()


def test_a_file_beyond_four_gigabytes():
    """2^32 + 2^20 bytes made on the device: one 64-byte row repeated behind a header padded to 64 bytes; five rows, two
    of them beyond 2^32 bytes, carry an id, a sequence and a sense of their own"""
    torch = pytest.importorskip("torch")
    total = (1 << 32) + (1 << 20)
    n = total // 64 - 1

    def make_row(r=None):
        rid, seq, sense = (b"g0000000", b"ACGTACGTACGTACGTACGT", b"-") if r is None else \
            (b"h%07d" % (r % 10**7), bytes(b"ACGT"[(r >> (2 * j)) & 3] for j in range(20)), b"+")
        row = rid + b"," + seq + b",NGG,chr1,123456789012345678901," + sense + b"\r\n"
        assert len(row) == 64
        return rid, seq, sense, row

    def on_device(data):
        return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    header = km.HEADER[:-1] + b" " * (63 - len(km.HEADER[:-1])) + b"\n"
    assert len(header) == 64
    buf = on_device(make_row()[3]).repeat(n + 1)
    assert buf.numel() == total
    buf[:64] = on_device(header)
    sampled = [0, 1 << 20, (1 << 26) - 1, (1 << 26) + 5, n - 1]
    for r in sampled:
        buf[64 * (r + 1):64 * (r + 2)] = on_device(make_row(r)[3])
    torch.cuda.synchronize()
    parsed = api.DeviceKmers.parse_device(buf.data_ptr(), total)
    try:
        assert (parsed.n, parsed.k, parsed.P, parsed.report["n_lines"]) == (n, 20, 3, n + 1)
        assert int(device_array(parsed.id_offsets_ptr + 8 * n, 1, np.uint64)[0]) == 8 * n
        for r in sampled + [5, n - 2]:
            rid, seq, sense, _ = make_row(r if r in sampled else None)
            assert device_array(parsed.ids_ptr + 8 * r, 8).tobytes() == rid, r
            assert int(device_array(parsed.id_offsets_ptr + 8 * r, 1, np.uint64)[0]) == 8 * r, r
            assert device_array(parsed.seqs_ptr + 20 * r, 20).tobytes() == seq, r
            assert device_array(parsed.pams_ptr + 3 * r, 3).tobytes() == b"NGG", r
            assert int(device_array(parsed.sense_positive_ptr + r, 1)[0]) == (1 if sense == b"+" else 0), r
    finally:
        parsed.close()
        del buf


def test_text_from_the_parsed_arrays_is_the_text_from_the_hosts_rows(toy):
    raw = (toy["dir"] / "kmers.csv").read_bytes()
    raw = b"".join(ln for ln in raw.splitlines(keepends=True) if not ln.startswith(b"nopam,"))   # one shape: 47 rows
    exp = km.parse(raw)
    assert len(exp.rows) == 47 and not exp.mixed
    gs = api.make_genome_structure(toy["names"], toy["lengths"])
    index = api.GenomeIndex.build(toy["text"], device=0)
    parsed = api.DeviceKmers.parse(raw)
    try:
        seqs = np.frombuffer(b"".join(r[1] for r in exp.rows), dtype=np.uint8).reshape(47, 20)
        pams = np.frombuffer(b"".join(r[2] for r in exp.rows), dtype=np.uint8).reshape(47, 3)
        for kw in (dict(), dict(sam=True), dict(mismatches=2, complete=False)):
            want = index.enumerate_text(seqs, pams, [r[0] for r in exp.rows], [r[3] for r in exp.rows], gs, **kw)
            got = index.enumerate_text_device(parsed.seqs_ptr, parsed.n, parsed.k, parsed.pams_ptr, parsed.P, parsed.ids_ptr,
                                              parsed.id_offsets_ptr, parsed.sense_positive_ptr, gs, **kw)
            assert len(want) > 1000 and got == want
    finally:
        parsed.close()
        index.close()

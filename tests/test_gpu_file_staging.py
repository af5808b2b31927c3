"""The one file-to-HBM staging loop (gs_staged_file, csrc/gs_scratch.h) from both of its callers, gs_fasta_parse_file and
gs_kmers_parse_file, at the sizes where it can go wrong.  With chunks of 4,096 bytes: no chunk, less than a chunk, a chunk
less a byte, exactly one chunk, a chunk and a byte, four chunks, four chunks and a byte - from the third chunk on the
reused event is waited for.  Each file read from its path must equal the model's expectation and the object parsed from
the same bytes in memory, errors included.  GPU only."""
import random
from importlib import import_module

import numpy as np
import pytest

import fasta_model as fm
import kmers_file_model as km

pytestmark = pytest.mark.gpu
api = import_module("guidescan-cli_amd.api")

CHUNK = 4096
SIZES = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 4 * CHUNK, 4 * CHUNK + 1)


def fasta_bytes(size):
    """titled records with CRLF line ends, blanks and both cases, cut to `size`"""
    raw, i = b"", 0
    while len(raw) < size:
        raw += b">r%d some words\r\n" % i + bytes(random.Random(i).choices(b"acgtnACGTN \r\n", k=700)) + b"\r\n"
        i += 1
    return raw[:size]


def kmers_bytes(size):
    """the header and rows; the last line has no newline and is padded with blanks to `size`"""
    last = b"last,ACGTACGTACGTACGTACGT,NGG,c,1,+"
    raw, i = km.HEADER, 0
    while len(raw) + len(km.row(i)) + len(last) <= size:
        raw, i = raw + km.row(i), i + 1
    raw += last
    return raw[:size] + b" " * (size - len(raw))


def outcome(make, read):
    """("ok", read(object)) or ("error", what the error carries)"""
    try:
        obj = make()
    except api.KmersFileError as e:
        return "error", (e.status, e.kind, e.message, e.line, e.row, e.offset, e.text)
    except api.GsError as e:
        return "error", (e.status, str(e))
    try:
        return "ok", read(obj)
    finally:
        obj.close()


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


@pytest.fixture
def chunks_of_4096():
    before = api.fasta_chunk_bytes(), api.kmers_chunk_bytes()
    try:
        assert api.fasta_chunk_bytes(CHUNK) == CHUNK and api.kmers_chunk_bytes(CHUNK) == CHUNK
        yield
    finally:
        api.fasta_chunk_bytes(before[0])
        api.kmers_chunk_bytes(before[1])


@pytest.mark.parametrize("size", SIZES)
def test_fasta_file_of(size, tmp_path, chunks_of_4096):
    raw = fasta_bytes(size)
    assert len(raw) == size and (size < CHUNK - 1 or (raw.count(b">") >= 5 and b"\r\n" in raw))
    p = tmp_path / "staged.fa"
    p.write_bytes(raw)
    exp = fm.expected(raw, tmp_path)
    for rules in ("index", "records"):
        def read(fa):
            return api._fasta_result(fa), fa.records(), fa.info(), set(fa.ms())

        from_path = outcome(lambda: api.DeviceFasta.parse(p, rules), read)
        from_memory = outcome(lambda: api.DeviceFasta.parse(raw, rules), read)
        where = f"{size} bytes, {rules} rules"
        assert from_path[0] == from_memory[0] and same(from_path[1], from_memory[1]), where
        if isinstance(exp[rules], fm.DuplicateRecord):
            assert from_path[0] == "error" and from_path[1][0] == 6, where
            assert f"FASTA record '{exp[rules].name.decode('latin-1')}' occurs twice" in from_path[1][1], where
            continue
        assert from_path[0] == "ok", (where, from_path[1])
        result, table, info, ms_keys = from_path[1]
        fm.compare(result, table, exp[rules], rules, where)
        assert ms_keys == {"read", "upload", "kernels", "names", "passes"}, where
        if size == 0:
            assert info == (0, 0, 0) and len(table["names"]) == 0, where


@pytest.mark.parametrize("size", SIZES)
def test_kmers_file_of(size, tmp_path, chunks_of_4096):
    raw = kmers_bytes(size)
    assert len(raw) == size
    p = tmp_path / "staged.csv"
    p.write_bytes(raw)

    def read(parsed):
        got = api.kmers_arrays(parsed)
        ms = got.pop("report")["ms"]
        assert set(ms) >= {"file_reads", "upload_waits", "device_stage"}, size
        return got

    from_path = outcome(lambda: api.DeviceKmers.parse(p), read)
    from_memory = outcome(lambda: api.DeviceKmers.parse(raw), read)
    assert from_path[0] == from_memory[0] and same(from_path[1], from_memory[1]), size
    try:
        exp = km.parse(raw)
    except km.KmersError as e:
        assert from_path[0] == "error" and from_path[1][:3] == (6, e.kind, e.message) and from_path[1][6] == e.text, size
        if e.kind in (km.FEW, km.POSITION):
            assert from_path[1][3:5] == (e.line, e.row), size
        if size == 0:
            assert from_path[1][:3] == (6, km.EMPTY, "empty kmers file")
        return
    assert size > 1 and not exp.mixed and len(exp.rows) >= 1
    assert from_path[0] == "ok", from_path[1]
    km.compare(from_path[1], exp, f"{size} bytes")


def test_a_directory_is_no_file(tmp_path):
    for parse in (lambda: api.DeviceFasta.parse(tmp_path, "index"), lambda: api.DeviceKmers.parse(tmp_path)):
        with pytest.raises(api.GsError) as e:
            parse()
        assert e.value.status == 5 and "cannot read" in str(e.value)

"""The device FASTA reader's summaries, composition and walk (csrc/gs_fasta_scan.h), run on the host through
gs_debug_fasta_host with tiles of 1, 2, 3, 7 and 64 bytes, against the two models of tests/fasta_model.py: the text, the
names, line_len, text_off and text_len of every record.  CPU only."""
from importlib import import_module

import pytest

import fasta_model as fm

api = import_module("guidescan-cli_amd.api")

TILES = (1, 2, 3, 7, 64)


def check_file(raw, tmp_path, what):
    exp = fm.expected(raw, tmp_path)
    for rules in ("index", "records"):
        for t in TILES:
            where = f"{what}, {rules} rules, tiles of {t}: {raw[:80]!r}"
            if isinstance(exp[rules], fm.DuplicateRecord):
                with pytest.raises(api.GsError) as e:
                    api.parse_fasta_model_tiles(raw, rules, t)
                assert e.value.status == 6, where
                assert f"FASTA record '{exp[rules].name.decode('latin-1')}' occurs twice" in str(e.value), where
                continue
            result, table = api.parse_fasta_model_tiles(raw, rules, t)
            fm.compare(result, table, exp[rules], rules, where)


@pytest.mark.parametrize("tile", TILES)
def test_tile_edge_files(tile, tmp_path):
    """the generator's files, made for this tile size and read with all five"""
    for name, raw in fm.tile_edge_files(tile).items():
        check_file(raw, tmp_path, f"{name} (made for {tile})")


def test_random_files(tmp_path):
    n = 0
    for raw in fm.random_files(2000, 300, seed=20240611):
        check_file(raw, tmp_path, f"random file {n}")
        n += 1
    assert n == 2000


def test_the_file_of_test_seqio(tmp_path):
    raw = b">chrA desc more\nacgtN\n  ACGT \n>chrB\nNNRY\n\n>empty\n"
    check_file(raw, tmp_path, "test_seqio's file")
    (text, names, lengths), _ = api.parse_fasta_model_tiles(raw, "index", 3)
    assert text.tobytes() == b"ACGTNACGTNNRY" and names == ["chrA", "chrB", "empty"] and lengths == [12, 4, 0]


def test_name_rules_are_the_host_readers(tmp_path):
    """the three places where `index`'s reader departs from seq_io.cxx stay as they are"""
    (_, names, _), _ = api.parse_fasta_model_tiles(b">chr1\r\nAC\r\n", "index", 2)
    assert names == ["chr1\r"]                       # a CRLF title without a space keeps its '\r'
    (_, names, _), _ = api.parse_fasta_model_tiles(b"> chr1\nAC\n", "index", 2)
    assert names == [""]                             # "> chr1" gives an empty name
    (text, names, lengths), _ = api.parse_fasta_model_tiles(b"ac\n>a\nGG\n", "index", 2)
    assert (text.tobytes(), names, lengths) == (b"ACGG", ["a"], [2])   # a first line that is no title: later records stand
    recs, _ = api.parse_fasta_model_tiles(b"> chr1 x\r\nA c\r\n>b\r\n", "records", 2)
    assert recs == {"chr1": b"Ac", "b": b""}


def test_duplicate_name_is_a_format_error_that_names_the_record():
    raw = b">a\nAC\n>b\nGG\n>a x\nTT\n>b\n"
    for t in TILES:
        with pytest.raises(api.GsError) as e:
            api.parse_fasta_model_tiles(raw, "records", t)
        assert e.value.status == 6 and "FASTA record 'a' occurs twice" in str(e.value)
        (text, names, _), _ = api.parse_fasta_model_tiles(raw, "index", t)     # no error under the index rules
        assert names == ["a", "b", "a", "b"] and text.tobytes() == b"ACGGTT"


def test_arguments():
    L = api.lib()
    import ctypes as C
    h = C.c_void_p()
    assert L.gs_debug_fasta_host(b"x", 1, 2, 4, C.byref(h)) == 1      # no such rule set
    assert L.gs_debug_fasta_host(b"x", 1, 0, 0, C.byref(h)) == 1      # no tile
    assert L.gs_fasta_parse(0, None, 5, 0, C.byref(h)) == 1
    assert L.gs_fasta_info(None, None, None, None) == 1
    assert api.fasta_tile_bytes() >= 16
    with api.DeviceFasta.host_model(b">a\nAC\n", "index", 2) as fa:
        with pytest.raises(api.GsError):
            fa.text_device_ptr()                                     # a host-made object has no device side

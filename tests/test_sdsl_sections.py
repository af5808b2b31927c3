"""The parts of the reference's index file that are functions of the text's 256 symbol counts alone - the serialised
_byte_tree (Huffman shape with its (frequency, node number) tie-breaking, breadth-first numbering, c_to_leaf, path) and
the serialised byte_alphabet - as the exporter (gs_sdsl_export.hip) restates them, against the files the reference
wrote: the toy index of tests/golden/toy (written by the reference's own `index` command) and, where oracle/_ref is
built, files written through the compiled reference containers for texts chosen to hit the tie-breaking.  CPU only."""
import os
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
from sdsl_walk import walk

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

ref = ol.ref()
needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref not built (no reference tree)")


def counts_of(text):
    c = np.bincount(np.asarray(text, dtype=np.uint8), minlength=256).astype(np.uint64)
    c[0] += 1   # the sentinel (sdsl/include/sdsl/construct.hpp:133-135)
    return c


def check_sections(buf, text):
    tree, alphabet = api.sdsl_sections(counts_of(text))
    assert buf.endswith(alphabet)
    sec, _ = walk(buf)
    assert sec["alphabet"] == (len(buf) - len(alphabet), len(buf))
    s, e = sec["tree"]
    assert buf[s:e] == tree
    assert buf.count(tree) == 1


@pytest.mark.parametrize("strand", ["forward", "reverse"])
def test_toy_tree_and_alphabet_sections(toy, strand):
    f = toy["dir"] / f"toy.idx.{strand}"
    check_sections(f.read_bytes(), api.sdsl_extract_text(f))


def _acgt(n_each):
    return np.tile(np.frombuffer(b"ACGT", np.uint8), n_each)


def _skewed():
    rng = np.random.default_rng(9)
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), 4000, p=[.9, .04, .03, .03])


def _exotic():
    from test_oracle_vs_ref import exotic_text
    return exotic_text()


TEXTS = {
    "two_symbols": lambda: np.random.default_rng(2).choice(np.frombuffer(b"AC", np.uint8), 700),
    "acgt_equal_counts": lambda: _acgt(64),
    "acgt_equal_counts_one_n": lambda: np.concatenate([_acgt(64), np.frombuffer(b"N", np.uint8)]),
    "exotic_alphabet": _exotic,
    "one_repeated_symbol": lambda: np.full(300, ord("G"), np.uint8),
    "skewed_90_percent_a": _skewed,
    "sentinel_ties_with_a_symbol": lambda: np.frombuffer(b"ACCGGGTTTT", np.uint8),
}


@needs_ref
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_sections_equal_the_compiled_reference(name, tmp_path):
    from test_oracle_vs_ref import make_ref_index
    text = np.ascontiguousarray(TEXTS[name](), dtype=np.uint8)
    n = text.shape[0] + 1
    oidx = ol.OracleIndex(text)
    try:
        for handle, strand_text in ((oidx.fwd, text), (oidx.rev, synth.reverse_complement_bytes(text))):
            h, _, _ = make_ref_index(handle, n)
            try:
                p = tmp_path / "x.idx"
                assert ref.ref_write_index_file(h, str(p).encode()) == 0
            finally:
                ref.ref_index_free(h)
            check_sections(p.read_bytes(), strand_text)
            os.unlink(p)
    finally:
        oidx.close()


def test_sections_reject_an_empty_alphabet():
    with pytest.raises(api.GsError):
        api.sdsl_sections(np.zeros(256, np.uint64))

"""The candidate-database entry points as far as they can be checked without a device: the header declares them and the
library exports them (gs_kmers_encode_ids, gs_kmers_get_ids, gs_kmers_csv, gs_kmers_concat, gs_format_device_ids,
gs_enumerate_text_device), NULL arguments are refused with GS_ERR_ARG before a device is touched, the CLI's usage text
names `kmers` and `--all-candidates`, and the new code reads no environment variable.  Runs on CPU."""
import ctypes as C
import re
import subprocess
from importlib import import_module

import numpy as np

import oracle_lib as ol

api = import_module("guidescan-cli_amd.api")
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
HEADER = ol.ROOT / "include" / "guidescan_amd.h"
NEW = ("gs_kmers_encode_ids", "gs_kmers_get_ids", "gs_kmers_csv", "gs_kmers_concat", "gs_format_device_ids",
       "gs_enumerate_text_device")
GS_ERR_ARG = 1


def test_the_header_declares_and_the_library_exports_the_entry_points():
    header = HEADER.read_text()
    L = api.lib()
    for name in NEW:
        assert re.search(r"\bgs_status\s+" + name + r"\s*\(", header), name
        assert name in api.EXPORTS
        assert getattr(L, name) is not None
    for method in ("format_device_ids", "enumerate_text_device", "raw_counts_device"):
        assert hasattr(api.GenomeIndex, method)
    for method in ("encode_ids", "ids_to_host", "csv"):
        assert hasattr(api.DeviceKmers, method)


def test_null_arguments_are_refused_without_a_device():
    L = api.lib()
    buf = C.create_string_buffer(b"A" * 64)  # stands for every array: a call that fails its checks reads none of them
    p = C.addressof(buf)
    g = api.make_genome_structure(["c"], [100])
    a, b, c, ln = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert L.gs_kmers_encode_ids(None, b"", b"chr1", None) == GS_ERR_ARG
    assert L.gs_kmers_get_ids(None, 1, C.byref(a), C.byref(b), C.byref(c)) == GS_ERR_ARG
    assert L.gs_kmers_get_ids(None, 0, C.byref(a), C.byref(b), C.byref(c)) == GS_ERR_ARG
    assert L.gs_kmers_csv(None, b"", b"chr1", C.byref(a), C.byref(ln)) == GS_ERR_ARG
    assert L.gs_kmers_concat(None, 2, C.byref(a)) == GS_ERR_ARG
    assert L.gs_kmers_concat((C.c_void_p * 2)(None, None), 2, C.byref(a)) == GS_ERR_ARG
    assert L.gs_kmers_concat((C.c_void_p * 1)(None), 0, None) == GS_ERR_ARG
    assert L.gs_format_device_ids(None, C.byref(g), p, 2, 20, p, 3, p, p, None, None, p, p, p, 3, 0, -1, None, C.byref(a),
                                  C.byref(ln)) == GS_ERR_ARG
    assert L.gs_enumerate_text_device(None, p, 2, 20, p, 3, None, 0, 3, 0, -1, C.byref(g), p, p, None, None, C.byref(a),
                                      C.byref(ln), None, None) == GS_ERR_ARG
    raw = np.zeros(2, np.uint32)
    assert L.gs_enumerate_text_device(None, p, 2, 20, p, 3, None, 0, 1, api.GS_FLAG_RAW_COUNTS, -1, C.byref(g), None, None, None,
                                      None, None, None, None, raw.ctypes.data) == GS_ERR_ARG
    assert a.value is None and ln.value == 0


def test_an_empty_concatenation_needs_no_device():
    """no parts: an empty object, made and freed on the host alone"""
    L = api.lib()
    h, n = C.c_void_p(), C.c_uint64(7)
    assert L.gs_kmers_concat(None, 0, C.byref(h)) == 0 and h.value
    assert L.gs_kmers_get(h, 1, C.byref(n), None, None, None, None) == 0 and n.value == 0
    assert L.gs_kmers_get_ids(h, 1, None, None, None) == GS_ERR_ARG  # no ids were encoded
    L.gs_kmers_free(h)


def test_usage_names_the_commands():
    r = subprocess.run([str(CLI)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    assert "guidescan kmers PREFIX -o KMERS" in r.stderr and "--all-candidates" in r.stderr and "--chromosomes" in r.stderr
    r = subprocess.run([str(CLI), "kmers"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage:" in r.stderr


def test_a_rejected_alt_pam_is_an_option_error_and_leaves_no_output_file(tmp_path):
    """-a takes 1 to 8 symbols: checked with the other options, before anything is read, built or created"""
    out = tmp_path / "o.csv"
    for bad in ("NNNNNNNNN", ""):
        r = subprocess.run([str(CLI), "enumerate", str(tmp_path / "no_such_index"), "-f", str(tmp_path / "no_such_kmers.csv"), "-o", str(out),
                            "-a", "NAG", "-a", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr == f"error: alt PAM {bad}: 1 to 8 symbols\n"
        assert not out.exists()


def test_the_new_code_reads_no_environment_variable():
    """tests/test_abi.py's rule (no getenv in the library) for the files this feature touches, and for every getenv of the
    CLI: --all-candidates and `kmers` added none (GS_ENCODER and GS_CLI_SAME_DEVICE were there before)"""
    csrc = ol.ROOT / "guidescan-cli_amd" / "csrc"
    for name in ("gs_kmers.hip", "gs_textdev.hip", "gs_host.hip"):
        assert not re.findall(r"\bgetenv\s*\(", (csrc / name).read_text()), name
    cli = "".join(p.read_text() for p in sorted((csrc / "host").iterdir()))  # the CLI is every file under host/
    assert len(re.findall(r"\bgetenv\b", cli)) == len(re.findall(r'getenv\("\w+"\)', cli))
    assert set(re.findall(r'getenv\("(\w+)"\)', cli)) == {"GS_ENCODER", "GS_CLI_SAME_DEVICE"}

"""The device text encoder's C-ABI as far as it can be checked without a device: the entry points are exported and
bound, a NULL handle is refused with GS_ERR_ARG (the other argument checks sit behind the handle check and are tested
on a live handle in tests/test_gpu_text_device.py), and the CLI's --encoder option accepts host|gpu only.  Runs on CPU."""
import ctypes as C
import os
import subprocess
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol

api = import_module("guidescan-cli_amd.api")
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
GS_ERR_ARG = 1


def test_both_entry_points_are_exported():
    L = api.lib()
    for name in ("gs_format_device", "gs_enumerate_text", "gs_index_last_text_offsets"):
        assert name in api.EXPORTS
        assert getattr(L, name) is not None
    assert hasattr(api.GenomeIndex, "format_device") and hasattr(api.GenomeIndex, "enumerate_text")
    assert b"0.3" in L.gs_version()


def test_a_null_handle_is_refused_without_a_device():
    """Only the handle check can be reached without a GPU: both entries test it first.  Every other NULL and size check
    needs a live handle and is exercised in tests/test_gpu_text_device.py (test_null_and_bad_size_arguments_*)."""
    g = api.make_genome_structure(["c"], [100])
    blob = C.create_string_buffer(b"ab")
    off = np.array([0, 1, 2], np.uint64)
    buf = C.create_string_buffer(b"A" * 64)  # stands for the arrays: a call that fails its handle check reads none of them
    p = C.addressof(buf)
    d_text, text, ln = C.c_void_p(), C.c_void_p(), C.c_uint64()
    L = api.lib()
    assert L.gs_format_device(None, C.byref(g), p, 2, 20, p, 3, C.addressof(blob), off.ctypes.data, None, None, p, p, p, 3, 0, -1,
                              None, C.byref(d_text), C.byref(ln)) == GS_ERR_ARG
    assert L.gs_enumerate_text(None, p, 2, 20, p, 3, None, 0, 3, 0, -1, C.byref(g), C.addressof(blob), off.ctypes.data, None, None,
                               C.byref(text), C.byref(ln), None) == GS_ERR_ARG
    out = np.zeros(3, np.uint64)
    assert L.gs_index_last_text_offsets(None, out.ctypes.data, 2) == GS_ERR_ARG
    assert d_text.value is None and text.value is None


@pytest.mark.parametrize("how", ["flag", "env"])
def test_cli_encoder_takes_host_or_gpu_only(tmp_path, how):
    args = [str(CLI), "enumerate", str(tmp_path / "x"), "-f", str(tmp_path / "k.csv"), "-o", str(tmp_path / "o.csv")]
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    if how == "flag":
        args += ["--encoder", "bogus"]
    else:
        env["GS_ENCODER"] = "bogus"
    r = subprocess.run(args, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2 and "usage:" in r.stderr and "--encoder host|gpu" in r.stderr
    assert not (tmp_path / "o.csv").exists()

"""No-GPU checks of the drop-in boundary: the shared library loads, exports every symbol the header
declares, the ctypes table matches the header, and argument errors are reported without a device."""
import ctypes
import os
import re

import pytest

from srcfinder_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "srcfinder_amd.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", src)


def test_header_declares_the_stage_api():
    names = declared_functions()
    for must in ["sf_cmf_run", "sf_cmf_score", "sf_cmf_loocv", "sf_cmf_eigh", "sf_cmf_covariance",
                 "sf_cmf_column_mean", "sf_cmf_extract_columns", "sf_cmf_filter", "sf_cmf_workspace_bytes"]:
        assert must in names


def test_library_exports_every_declared_symbol():
    assert os.path.isfile(_ffi.LIB_PATH), "build the HIP library first (__graft_entry__.build())"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in declared_functions():
        assert hasattr(L, name), "libsrcfinder_amd.so does not export %s" % name


def test_ctypes_table_matches_header():
    names = set(declared_functions())
    assert names == set(_ffi.SIGNATURES), names ^ set(_ffi.SIGNATURES)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (_, args) in _ffi.SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else len(params.split(","))
        assert n == len(args), "%s: header has %d parameters, ctypes table %d" % (name, n, len(args))


def test_host_only_entry_points():
    L = _ffi.lib()
    assert L.sf_version() >= 100
    nbytes = L.sf_cmf_workspace_bytes(20000, 72, 598, 201)
    # xt (598*20000*72*4 = 3.44 GB) dominates
    assert 3.4e9 < nbytes < 6e9
    assert L.sf_cmf_workspace_bytes(0, 72, 598, 201) == 0


def test_argument_errors_do_not_touch_the_device():
    L = _ffi.lib()
    one = ctypes.c_void_p(16)
    # bad shard
    rc = L.sf_cmf_extract_columns(one, 10, 425, 64, 5, 3, 350, 72, one, one, None)
    assert rc < 0 and b"column shard" in L.sf_last_error_string()
    # bad window
    rc = L.sf_cmf_extract_columns(one, 10, 425, 64, 0, 64, 400, 72, one, one, None)
    assert rc < 0 and b"active window" in L.sf_last_error_string()
    # nodata > 0 must be refused like the reference does (robust_mf.py:232-234)
    rc = L.sf_cmf_score(one, 10, 425, 64, 0, 64, 350, 72, one, one, one, one, one, 60, 42, 24, 1.0,
                        one, 64, 0, 4, None, None, None, None)
    assert rc == -3 and b"nodata" in L.sf_last_error_string()


def test_python_surface_rejects_what_the_reference_rejects():
    from srcfinder_amd import cmf
    assert cmf.active_window("ch4") == (351, 422)
    assert cmf.active_window("ch4", True) == (5, 420)
    assert cmf.active_window("co2") == (309, 391)
    with pytest.raises(ValueError):
        cmf.active_window("n2o")
    a = cmf.alpha_grid()
    assert len(a) == 201 and a[0] == 1e-10 and a[200] == 1.0000000000003273
    assert cmf.model_parameters(False, (351, 422)) == (
        "{ modelname=looshrinkage, bgmodel=unimodal, aminexp=-10.0, amaxexp=0.0, astep=0.05, "
        "reflectance=False, active_bands=[351, 422] }")


def test_model_parameter_string_matches_reference_run(golden_dir):
    import numpy as np
    from srcfinder_amd import cmf
    g = np.load(os.path.join(golden_dir, "cmf_S_radiance.npz"))
    assert str(g["modelparms"]) == cmf.model_parameters(False, (351, 422))
    g = np.load(os.path.join(golden_dir, "cmf_R_reflectance.npz"))
    assert str(g["modelparms"]) == cmf.model_parameters(True, (5, 420))


def test_product_fails_loudly_without_library_or_gpu(monkeypatch, tmp_path):
    """No CPU fallback: a missing libsrcfinder_amd.so raises from _ffi.lib(), and with no GPU visible the mirror raises
    before any computation; nothing under srcfinder_amd/ imports the oracle."""
    import numpy as np
    import torch
    from srcfinder_amd import cmf, cnn
    monkeypatch.setattr(_ffi, "_lib", None)
    monkeypatch.setattr(_ffi, "LIB_PATH", str(tmp_path / "libsrcfinder_amd.so"))
    with pytest.raises(_ffi.SrcfinderError, match="no CPU fallback"):
        _ffi.lib()
    if not torch.cuda.is_available():
        with pytest.raises(_ffi.SrcfinderError, match="no GPU visible"):
            cmf.robust_mf(np.zeros((4, 425, 2), np.float32), np.zeros((425, 3)))
        with pytest.raises(_ffi.SrcfinderError):
            cnn.predict_flightline(np.zeros((3, 3), np.float32), weights={})
    pkg = os.path.join(ROOT, "srcfinder_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn


def test_tuning_knobs_refuse_retired_forms_and_stay_per_thread():
    """sf_debug_set refuses a retired key and a retired value of a kept key (an A/B run would otherwise measure the default
    twice), takes every value the suite, smoke() and bench.py set, and changes only the calling thread's knobs."""
    import threading
    L = _ffi.lib()
    got = ctypes.c_int(0)
    for key in (4, 5, 8, 19, 26):                                   # retired keys: unknown, as any other unknown key
        assert L.sf_debug_set(key, 0) == -1 and L.sf_debug_set(key, 1) == -1, key
        assert b"unknown key" in L.sf_last_error_string()
        assert L.sf_debug_get(key, ctypes.byref(got)) == -1, key
    retired = {6: (2, 3, 5, 7, 9), 7: (4, 8, 16), 15: (2,), 16: (2, 4), 17: (10, 11, 12, 14, 25), 20: (2, 3, 100, 101, 196),
               2: (-1,)}
    for key, values in retired.items():
        for v in values:
            assert L.sf_debug_set(key, v) == -1, (key, v)
            msg = L.sf_last_error_string()
            assert b"key %d" % key in msg and b"%d" % v in msg, msg
            assert L.sf_debug_get(key, ctypes.byref(got)) == 0 and got.value == 0, (key, v)   # the refusal changed nothing
    used = {1: (0, 5, 7, 100, 200), 2: (0, 4, 64), 3: (0, 1), 6: (0, 1), 7: (0, 2), 10: (0, 1, 6, 7, 8), 14: (0, 1), 15: (0, 1),
            16: (0, 1, 3), 17: (0, 1, 2, 4), 18: (0, 1, 2, 3), 20: (0, 1, 4, 5), 21: (0, 1), 22: (0, 1), 24: (0, 1, 2, 4, 5)}
    for key, values in used.items():
        before = ctypes.c_int(0)
        assert L.sf_debug_get(key, ctypes.byref(before)) == 0, key
        for v in values:
            assert L.sf_debug_set(key, v) == 0, (key, v, L.sf_last_error_string())
            assert L.sf_debug_get(key, ctypes.byref(got)) == 0 and got.value == v, (key, v)
        assert L.sf_debug_set(key, before.value) == 0
    # per calling thread: a knob set here is not seen by another thread, and one set there does not reach this one
    seen = {}

    def other():
        v = ctypes.c_int(-1)
        L.sf_debug_get(20, ctypes.byref(v))
        seen["before"] = v.value
        L.sf_debug_set(20, 4)
        L.sf_debug_get(20, ctypes.byref(v))
        seen["after"] = v.value

    assert L.sf_debug_set(20, 1) == 0
    try:
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert L.sf_debug_get(20, ctypes.byref(got)) == 0 and got.value == 1
    finally:
        L.sf_debug_set(20, 0)
    assert seen == {"before": 0, "after": 4}


def test_cnn_score_workspace_bytes_is_the_need_of_every_route():
    """sf_cnn_score_rows checks the workspace against the layout the call will build (route 0: the trunk shared through
    inception3b, depth 2; route 5: through conv3, depth 1; the others share nothing), and sf_cnn_score_workspace_bytes(batch, H, W,
    route) reports exactly that need.  Where no depth-2 strip fits under the 2 GB map + ring limit, depth 2 shares nothing but depth 1
    still does: the depth-1 buffers must be counted (before, a workspace of the reported size was written past its end).  A 1-byte
    workspace: every call returns -4 at the size check, before any device work, so the dummy pointers are never read."""
    L = _ffi.lib()
    one = ctypes.c_void_p(16)
    H = 1000
    for batch in (64, 1024, 2048, 4096):
        base = L.sf_cnn_score_workspace_bytes(batch, 0, 0, 0)
        for W in (300, 598, 1242, 2400):
            for route in (0, 5, 3, 4, 2, 1):
                assert L.sf_cnn_score_workspace_bytes(batch, 0, 0, route) == base, (batch, route)
                rc = L.sf_cnn_score_rows(one, one, H, W, 0, H, one, one, batch, route, None, None, one, 1, None)
                msg = L.sf_last_error_string().decode()
                assert rc == -4, (batch, W, route, rc, msg)
                m = re.search(r"need (\d+) bytes, got 1\b", msg)
                assert m, msg
                need = int(m.group(1))
                assert need == L.sf_cnn_score_workspace_bytes(batch, H, W, route), (batch, W, route, need)
                assert need >= base and (route in (0, 5) or need == base), (batch, W, route, need, base)
                if (batch, W) in ((2048, 1242), (4096, 598)) and route == 5:
                    assert need > base, (batch, W, need, base)      # the depth-1 maps and rings are counted
    for route in (-1, 6):                                           # not a route: no size, and the call refuses it
        assert L.sf_cnn_score_workspace_bytes(64, H, 300, route) == 0
        assert L.sf_cnn_score_rows(one, one, H, 300, 0, H, one, one, 64, route, None, None, one, 1, None) == -1

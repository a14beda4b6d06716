"""No-GPU checks of the pixel-set scorer and the per-plume saliency: the two entries are declared, exported and in the ctypes table,
sf_cnn_score_pixels refuses bad arguments before it touches a device, and the command lines take the new flags."""
import ctypes
import os
import re

from srcfinder_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "srcfinder_amd.h")
NEW = ("sf_cnn_score_pixels", "sf_plumes_saliency")


def test_new_entries_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        assert hasattr(L, name), name
        assert name in _ffi.SIGNATURES
        assert len(m.group(1).split(",")) == len(_ffi.SIGNATURES[name][1]), name
    assert len(_ffi.SIGNATURES["sf_cnn_score_pixels"][1]) == 15


def _score_pixels(L, padded=16, npix=4, route=3, batch=8, ws_bytes=None):
    one = ctypes.c_void_p(16)
    if ws_bytes is None:
        ws_bytes = L.sf_cnn_score_workspace_bytes(batch, 0, 0, 3)
    info = (ctypes.c_int * 2)(7, 7)
    rc = L.sf_cnn_score_pixels(None if padded is None else ctypes.c_void_p(padded), one, 20, 30, one, ctypes.c_longlong(npix), one,
                               one, batch, route, None, info, one, ctypes.c_size_t(ws_bytes), None)
    return rc, info


def test_score_pixels_argument_errors_do_not_touch_the_device():
    L = _ffi.lib()
    rc, _ = _score_pixels(L, padded=None)
    assert rc == -1 and b"sf_cnn_score_pixels" in L.sf_last_error_string()
    rc, _ = _score_pixels(L, npix=-1)
    assert rc == -1
    for route in (0, 5):
        rc, _ = _score_pixels(L, route=route)
        assert rc == -1 and b"route 3" in L.sf_last_error_string(), route
    rc, _ = _score_pixels(L, route=6)
    assert rc == -1
    rc, _ = _score_pixels(L, batch=0)
    assert rc == -1
    need = L.sf_cnn_score_workspace_bytes(8, 0, 0, 3)
    assert need > 0
    rc, _ = _score_pixels(L, ws_bytes=need - 1)
    assert rc == -4 and b"workspace too small" in L.sf_last_error_string()
    rc, info = _score_pixels(L, npix=0)
    assert rc == 0 and list(info) == [0, 0]


def test_plumes_saliency_argument_errors_do_not_touch_the_device():
    L = _ffi.lib()
    one = ctypes.c_void_p(16)
    assert L.sf_plumes_saliency(one, None, 4, 4, 1, one, one, one, None) == -1
    assert L.sf_plumes_saliency(one, one, 4, 4, -1, one, one, one, None) == -1
    assert L.sf_plumes_saliency(one, one, 0, 4, 1, one, one, one, None) == -1


def test_command_lines_take_the_new_flags():
    from srcfinder_amd import cli_cnn_pred, cli_filtdet
    a = cli_cnn_pred.build_parser().parse_args(["fl.img", "--mask", "fl_ccomp"])
    assert a.mask == "fl_ccomp"
    assert cli_cnn_pred.build_parser().parse_args(["fl.img"]).mask is None
    b = cli_filtdet.build_parser().parse_args(["cmf.img", "out", "--weights", "w.pt", "--model", "Permian_QC", "--batch", "512"])
    assert (b.weights, b.model, b.batch) == ("w.pt", "Permian_QC", 512)
    c = cli_filtdet.build_parser().parse_args(["cmf.img", "out"])
    assert (c.weights, c.model, c.batch) == (None, "COVID_QC", 1024)

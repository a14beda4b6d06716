"""The CNN tile scorer on a pixel set (sf_cnn_score_pixels, predict_flightline(mask=...)) and the per-plume saliency
(sf_plumes_saliency, plume_table(saliency=...), cli_filtdet --weights, cli_cnn_pred --mask).

A window's bits do not depend on its batch or on trunk sharing, and the activation scales are calibrated on fixed windows of the
plane: a masked map equals the full map at the mask bit for bit (when neither call scored a batch again), and the filled golden
pins it to the reference."""
import csv
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from srcfinder_amd import cnn  # noqa: E402
from srcfinder_amd.cnn_weights import synthetic_plane, synthetic_state_dict  # noqa: E402

MEAN, STD = cnn.MODEL_NORM["COVID_QC"]


@pytest.fixture(scope="module")
def net():
    import torch
    assert torch.cuda.is_available()
    return cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024))


@pytest.fixture(scope="module")
def filled(golden_dir):
    return np.load(os.path.join(golden_dir, "cnn_googlenet_filled_golden.npz"))


def _filled_plane(g, key):
    from srcfinder_amd import cnn_weights
    plane = getattr(cnn_weights, str(g[key + "_gen"]))(int(g[key + "_H"]), int(g[key + "_W"]), seed=int(g[key + "_seed"]))
    for r, c in g[key + "_nodata"]:
        plane[r, c] = -9999.0
    return plane


def _p_error(got, want, what):
    """max |d| / min(p, 1 - p) over the data windows; asserts NODATA placement and |d| <= 1e-4 min(p, 1 - p) + 1e-7."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(got == -9999, want == -9999), what
    v = want != -9999
    d, m = np.abs(got[v] - want[v]), np.minimum(want[v], 1 - want[v])
    worst = float((d / m).max())
    assert np.all(d <= 1e-4 * m + 1e-7), (what, worst, int(np.argmax(d / m)))
    return worst


def _mask(shape, idx):
    m = np.zeros(int(np.prod(shape)), dtype=bool)
    m[np.asarray(idx, dtype=np.int64)] = True
    return m.reshape(shape)


@pytest.fixture(scope="module")
def full_maps(filled, net):
    """The full map of planes A and B (route "split": the shared trunk), none of its batches scored again."""
    maps = {}
    for key in ("A", "B"):
        info = {}
        plane = _filled_plane(filled, key)
        maps[key] = (plane, cnn.predict_flightline(plane, (MEAN, STD), net=net, route="split", batch=512, lanes=1, info=info))
        assert info["rescued_batches"] == 0, (key, info)
    return maps


@pytest.mark.parametrize("route", ["split", "winograd"])
@pytest.mark.parametrize("batch", [512, 7])
def test_masked_windows_against_the_reference_on_filled_planes(filled, net, route, batch):
    for key in ("A", "B"):
        plane, idx = _filled_plane(filled, key), filled[key + "_idx"]
        m = _mask(plane.shape, idx)
        info = {}
        got = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, route=route, mask=m, info=info, to_numpy=True)
        assert info["route"] == (3 if route == "split" else 4) and info["pixels"] == int(m.sum()), info
        _p_error(got.reshape(-1)[idx], filled[key + "_prob"], (route, batch, key))
        assert np.all(got[~m] == 0), (route, batch, key)


def test_masked_map_equals_the_full_map_bit_for_bit(full_maps, filled, net):
    import torch
    rng = np.random.default_rng(11)
    for key in ("A", "B"):
        plane, full = full_maps[key]
        H, W = plane.shape
        idx = filled[key + "_idx"]
        edge = [0, W - 1, (H - 1) * W, H * W - 1, W // 2, (H - 1) * W + W // 2, (H // 2) * W, (H // 2) * W + W - 1]
        rand = np.concatenate([rng.choice(H * W, 5000, replace=False), edge])
        row = np.arange(W) + (H // 3) * W
        for what, pix, batch in (("pinned", idx, 512), ("random", rand, 512), ("pinned, batch 1", idx, 1), ("one row", row, 512)):
            m = _mask((H, W), pix)
            info = {}
            got = cnn.predict_flightline(plane, (MEAN, STD), net=net, route="split", batch=batch, mask=m, info=info)
            assert info["rescued_batches"] == 0, (key, what, info)
            mt = torch.as_tensor(m, device=got.device)
            assert torch.equal(got[mt], full[mt]), (key, what)
            assert torch.equal(got[~mt], torch.zeros_like(got[~mt])), (key, what)
        # the same pixels through the ABI in reverse order and with duplicates: the same map
        ds = cnn.FlightlineConvolve(plane, (MEAN, STD), device=net.device)
        net.calibrate(ds, 512)
        outs = []
        for order in (np.sort(rand), np.concatenate([rand[::-1], rand[:700], rand[-5:]])):
            out = torch.zeros(H * W, dtype=torch.float32, device=net.device)
            pix = torch.as_tensor(order.astype(np.int64), device=net.device)
            assert cnn._score_pixels_c(net, ds, pix, 512, out, 3) == 0
            outs.append(out.view(H, W))
        assert torch.equal(outs[0], outs[1]), key
        mt = torch.as_tensor(_mask((H, W), rand), device=net.device)
        assert torch.equal(outs[0][mt], full[mt]), key


def test_masked_overflow_is_rescued_inside_the_call():
    """The setup of test_cnn_gpu's overflow test (weights blown up by 1e5, scales pinned to 1): every masked batch overflows float16,
    is scored again on the fp32 matrix cores inside the call, with a warning -- the same bits as route "winograd" on the mask."""
    import torch
    from srcfinder_amd import _ffi
    sd = synthetic_state_dict(seed=7)
    sd = {k: (v * 1e5 if k == "conv1.conv.weight" else v) for k, v in sd.items()}
    net = cnn.GoogLeNetHIP(sd)
    plane = synthetic_plane(6, 5, seed=2)
    ones = [1.0] * _ffi.lib().sf_cnn_num_scales()
    m = _mask(plane.shape, [0, 3, 7, 8, 11, 12, 19, 23, 24, 29])
    want = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=4, route="winograd", mask=m)
    info = {}
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        got = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=4, scales=ones, mask=m, info=info)
    assert any("float16 range" in str(w.message) for w in wlist)
    assert info["rescued_batches"] >= 1 and info["batches"] == 3 and info["route"] == 3, info
    assert torch.equal(got, want)


def test_masked_gpu_list_and_refusals(full_maps, filled, net):
    import torch
    plane, _ = full_maps["B"]
    m = _mask(plane.shape, filled["B_idx"])
    sd = synthetic_state_dict(seed=2024)
    a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=16, mask=m)
    info = {}
    b = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=16, gpus=[0, 0, 0], mask=torch.as_tensor(m).cuda(), info=info)
    assert torch.equal(a, b) and info["pixels"] == int(m.sum()) and info["rescued_batches"] == 0
    with pytest.raises(ValueError):
        cnn.predict_flightline(plane, (MEAN, STD), net=net, rows=(0, 4), mask=m)
    with pytest.raises(ValueError):
        cnn.predict_flightline(plane, (MEAN, STD), net=net, mask=m[:-1])
    with pytest.raises(ValueError):
        cnn.predict_flightline(plane, (MEAN, STD), weights=sd, precision="fp16", mask=m)


def _reference_saliency_columns(detcomp, sal):
    """numpy: per component the max saliency over its pixels that are not -9999 and the first (row, col) of it in raster order."""
    W = detcomp.shape[1]
    out = []
    for i in range(1, int(detcomp.max()) + 1):
        sel = np.flatnonzero((detcomp.reshape(-1) == i) & (sal.reshape(-1) != -9999))
        if sel.size == 0:
            out.append((float("nan"), -1, -1))
            continue
        k = int(sel[np.argmax(sal.reshape(-1)[sel])])
        out.append((float(sal.reshape(-1)[k]), k // W, k % W))
    return out


def test_plume_saliency_on_filtdet_components(net):
    import torch
    from srcfinder_amd import plumes, synth
    ch4mf = synth.make_cmf_plane(400, 300, nplumes=12, seed=21)
    nodata = ch4mf == -9999
    _, detcomp = plumes.filtdet(ch4mf, nodata)
    comp = detcomp.cpu().numpy()
    assert comp.max() >= 5
    plane = ch4mf.astype(np.float32)
    info, finfo = {}, {}
    sal = cnn.predict_flightline(plane, "COVID_QC", net=net, batch=1024, mask=detcomp > 0, info=info)
    full = cnn.predict_flightline(plane, "COVID_QC", net=net, batch=1024, route="split", info=finfo)
    assert info["rescued_batches"] == 0 and finfo["rescued_batches"] == 0
    inside = detcomp > 0
    assert torch.equal(sal[inside], full[inside]) and bool((sal[~inside] == 0).all())
    header, rows = plumes.plume_table(ch4mf, detcomp, saliency=sal)
    assert header == plumes.HEADER + ["salmax", "salmaxrow", "salmaxcol"]
    want = _reference_saliency_columns(comp, sal.cpu().numpy())
    assert len(rows) == len(want)
    for r, w in zip(rows, want):
        assert (r[-3], r[-2], r[-1]) == w, (r, w)
    h0, rows0 = plumes.plume_table(ch4mf, detcomp)
    assert h0 == plumes.HEADER and [repr(r[:len(h0)]) for r in rows] == [repr(r) for r in rows0]     # (lat / lon: NaN)


def test_plume_saliency_rules_on_a_hand_made_map():
    """sf_plumes_saliency's own rules on a constructed map (filtdet's components never hold CNN NODATA): -9999 is skipped -- at a
    component's first raster pixel and where its largest value would be --, a component without a scored pixel gets NaN, -1, -1,
    equal maxima go to the first in raster order, and pixels of the background or of another component inside a bounding box do not
    count."""
    from srcfinder_amd import plumes
    H, W = 24, 30
    comp = np.zeros((H, W), np.int32)
    comp[2:8, 3:12] = 1
    comp[10:14, 2:6] = 2
    comp[15:22, 8:20] = 3
    comp[17:19, 12:15] = 4                 # inside 3's bounding box
    comp[16, 10] = 0                       # a hole of 3
    rng = np.random.default_rng(3)
    sal = rng.uniform(0.0, 0.9, (H, W)).astype(np.float32)
    sal[2, 3] = -9999.0                    # 1: its first raster pixel
    sal[5, 7] = -9999.0                    # 1: where its largest value would be
    sal[4, 9] = 0.93                       # 1: the largest scored value
    sal[10:14, 2:6] = -9999.0              # 2: nothing scored
    sal[16, 18] = sal[20, 9] = 0.97        # 3: two equal maxima
    sal[16, 10] = 1.0                      # 3's hole (background)
    sal[17, 13] = 0.99                     # 4, inside 3's box
    sal[0, 0] = 1.0                        # background
    ch4mf = np.full((H, W), 700.0)
    header, rows = plumes.plume_table(ch4mf, comp, saliency=sal)
    assert header[-3:] == ["salmax", "salmaxrow", "salmaxcol"] and len(rows) == 4
    got = [(r[-3], r[-2], r[-1]) for r in rows]
    want = _reference_saliency_columns(comp, sal)
    assert np.isnan(got[1][0]) and got[1][1:] == (-1, -1) and np.isnan(want[1][0])
    for i in (0, 2, 3):
        assert got[i] == want[i], (i, got[i], want[i])
    assert got[0] == (float(np.float32(0.93)), 4, 9)
    assert got[2] == (float(np.float32(0.97)), 16, 18)
    assert got[3] == (float(np.float32(0.99)), 17, 13)


def _product(path, ch4mf):
    from srcfinder_amd import envi
    H, W = ch4mf.shape
    mm = envi.create_image(path, {"lines": H, "samples": W, "bands": 4}, np.float64, "bip")
    mm[..., :3] = np.where((ch4mf == -9999)[..., None], -9999.0, 1.0)
    mm[..., 3] = ch4mf
    mm.flush()
    del mm


def test_command_lines_with_the_cnn_on_plume_pixels(tmp_path):
    import torch
    from srcfinder_amd import cli_cnn_pred, cli_filtdet, envi, plumes, synth
    ch4mf = synth.make_cmf_plane(160, 120, nplumes=6, seed=5)
    stem = "ang20200101t000000_cmf_img"
    path = str(tmp_path / stem)
    _product(path, ch4mf)
    sd = synthetic_state_dict(seed=2024)
    wpath = str(tmp_path / "COVID_QC.pt")
    torch.save({k: torch.as_tensor(v) for k, v in sd.items()}, wpath)
    # what the CLI must reproduce, from the functions
    _, detcomp = plumes.filtdet(ch4mf, ch4mf == -9999)
    assert int(detcomp.max()) >= 2
    sal = cnn.predict_flightline(ch4mf.astype(np.float32), "COVID_QC", weights=sd, batch=1024, mask=detcomp > 0)
    header, rows = plumes.plume_table(ch4mf, detcomp, lid=stem, saliency=sal)
    out = tmp_path / "out"
    assert cli_filtdet.main([path, str(out), "--weights", wpath, "--model", "COVID_QC", "--batch", "1024"]) == 0
    got = list(csv.reader(open(str(out / (stem + "_plumes.csv")))))
    assert got[0] == header and got[0][-3:] == ["salmax", "salmaxrow", "salmaxcol"] and len(got) - 1 == len(rows)
    for g, r in zip(got[1:], rows):
        assert float(g[-3]) == r[-3] and int(g[-2]) == r[-2] and int(g[-1]) == r[-1], (g, r)
    smap, smeta = envi.open_memmap(str(out / (stem + "_saliency")))
    assert (smeta["bands"], smeta["data type"]) == (1, 4)
    assert np.array_equal(np.asarray(smap[0]), sal.cpu().numpy())
    # without --weights: no saliency image, the table of today
    out0 = tmp_path / "out0"
    assert cli_filtdet.main([path, str(out0)]) == 0
    assert not any(p.startswith(stem + "_saliency") for p in os.listdir(str(out0)))
    assert next(csv.reader(open(str(out0 / (stem + "_plumes.csv"))))) == plumes.HEADER
    # cli_cnn_pred --mask <stem>_ccomp: the component pixels (>= 1; background 0, NODATA -9999)
    ccomp = str(out / (stem + "_ccomp"))
    assert cli_cnn_pred.main([path, "-g", "0", "-o", str(tmp_path), "--band", "4", "--weights", wpath, "--mask", ccomp]) == 0
    cmap, _ = envi.open_memmap(str(tmp_path / (stem + "_saliency.img")))
    cc = np.asarray(envi.open_memmap(ccomp)[0][0])
    want = cnn.predict_flightline(ch4mf.astype(np.float32), "COVID_QC", weights=sd, batch=1024, mask=cc > 0, to_numpy=True)
    assert np.array_equal(np.asarray(cmap[0]), want)
    assert np.array_equal(want, sal.cpu().numpy())
    # a mask of another shape
    bad = str(tmp_path / "bad_mask")
    mm = envi.create_image(bad, {"lines": 10, "samples": 120, "bands": 1}, np.float32, "bsq")
    mm[...] = 1
    mm.flush()
    del mm
    assert cli_cnn_pred.main([path, "-g", "0", "-o", str(tmp_path), "--band", "4", "--weights", wpath, "--mask", bad]) == 1

"""The CMF-threshold plume detector on the GPU against the reference's goldens (tests/golden/gen_golden_filtdet.py) and
against the numpy / scipy restatement of tests/test_plumes_cpu.py on a full 598-sample x 20000-line plane."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

from test_plumes_cpu import filtdet_np, golden_params, load_golden, prestage, table_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir)


def _run(ch4mf, nodata, **p):
    from srcfinder_amd import plumes
    kde, comp = plumes.filtdet(ch4mf, nodata, **p)
    return kde.cpu().numpy(), comp.cpu().numpy()


def _check_table(ch4mf, comp, mapinfo, want_int, want_f, ps):
    from srcfinder_amd import plumes
    header, rows = plumes.plume_table(ch4mf, comp, mapinfo)
    assert len(rows) == len(want_int)
    ix = {h: i for i, h in enumerate(header)}
    got_int = np.array([[r[ix[c]] for c in ("npix", "bbminr", "bbmaxr", "bbminc", "bbmaxc", "ppmmmaxrow", "ppmmmaxcol")]
                        for r in rows], np.int64).reshape(-1, 7)
    got_f = np.array([[r[ix["ppmmsum"]], r[ix["ppmmmax"]], r[ix["ime_kg"]]] for r in rows]).reshape(-1, 3)
    assert np.array_equal(got_int, want_int)
    assert np.allclose(got_f, want_f, rtol=1e-12, atol=0)
    return header, rows


def test_every_reference_golden(golden):
    from srcfinder_amd import detections
    mi = detections.mapinfo(list(golden["mapinfo"]))
    for name in golden["scenes"]:
        ch4mf, nodata = golden["%s_ch4mf" % name], golden["%s_nodata" % name]
        kde, comp = _run(ch4mf, nodata, **golden_params(golden, name))
        assert comp.dtype == np.int32
        assert np.array_equal(comp, golden["%s_detcomp" % name]), name
        assert np.allclose(kde, golden["%s_detkde" % name], rtol=1e-12, atol=1e-300), name
        header, rows = _check_table(ch4mf, comp, mi, golden["%s_table_int" % name], golden["%s_table_f" % name],
                                    float(golden["ps"]))
        for r in rows:                                  # the max's lat / lon through detections.sl2latlon
            lat, lon = detections.sl2latlon(r[header.index("ppmmmaxcol")], r[header.index("ppmmmaxrow")], mi)
            assert r[header.index("ppmmmaxlat")] == float(np.asarray(lat).reshape(-1)[0])
            assert r[header.index("ppmmmaxlon")] == float(np.asarray(lon).reshape(-1)[0])


@pytest.fixture(scope="module")
def big_plane():
    from srcfinder_amd.synth import make_cmf_plane
    img = make_cmf_plane(20000, 598, seed=2026)
    return img, img == -9999


def test_full_plane_against_restatement_and_deterministic(big_plane):
    img, nodata = big_plane
    pre = prestage(img, 50, False, False)
    assert (np.abs(pre - 500) / 500).min() > 1e-9                # the margin: no pixel can flip on blur rounding
    want_kde, want_comp = filtdet_np(img, nodata)
    assert want_comp.max() > 100
    kde1, comp1 = _run(img, nodata)
    assert np.array_equal(comp1, want_comp)
    # 1e-12 of the pre-clip value: a pixel just above mfmin has a tiny detkde = (d - mfmin) / (mfmax - mfmin), whose own
    # relative error is the blur's rounding of d over that small difference
    err = np.abs(kde1 - want_kde)
    bound = 1e-12 * (np.abs(want_kde) + 1500.0 / 1000.0)
    assert (err <= bound).all(), "max |d detkde| %.3e, max relative %.3e" % (err.max(), (err / np.maximum(want_kde, 1e-300)).max())
    kde2, comp2 = _run(img, nodata)
    assert np.array_equal(comp1, comp2) and np.array_equal(kde1.view(np.int64), kde2.view(np.int64))
    from srcfinder_amd import plumes
    h, r1 = plumes.plume_table(img, comp1, {"xps": 5.0})
    h, r2 = plumes.plume_table(img, comp1, {"xps": 5.0})
    num = [i for i, c in enumerate(h) if c not in ("plumeid", "lid")]
    a1 = np.array([[r[i] for i in num] for r in r1], np.float64)
    a2 = np.array([[r[i] for i in num] for r in r2], np.float64)
    assert np.array_equal(a1.view(np.int64), a2.view(np.int64))   # bit-identical sums: no float atomics
    want_int, want_f = table_np(img, want_comp, 5.0)
    _check_table(img, comp1, {"xps": 5.0}, want_int, want_f, 5.0)


def test_label4_and_label8_against_scipy():
    import torch
    from srcfinder_amd import _ffi
    L = _ffi.lib()
    rng = np.random.default_rng(5)
    for H, W, p in [(1, 1, 1.0), (7, 300, 0.5), (300, 7, 0.55), (257, 129, 0.45), (64, 64, 0.6)]:
        m = rng.random((H, W)) < p
        md = torch.as_tensor(m.astype(np.uint8)).cuda()
        scratch = torch.empty(L.sf_image_label8_scratch_bytes(H, W), dtype=torch.uint8, device="cuda")
        for fn, conn in ((L.sf_image_label4, 1), (L.sf_image_label8, 2)):
            lab = torch.empty((H, W), dtype=torch.int32, device="cuda")
            n = torch.empty(1, dtype=torch.int32, device="cuda")
            area = torch.empty(H * W + 2, dtype=torch.int32, device="cuda")
            _ffi.check(fn(_ffi.ptr(md), H, W, _ffi.ptr(lab), _ffi.ptr(area), H * W + 2, _ffi.ptr(n), _ffi.ptr(scratch),
                          _ffi.stream_ptr()), "label")
            want, nw = ndi.label(m, structure=ndi.generate_binary_structure(2, conn))
            assert np.array_equal(lab.cpu().numpy(), want) and int(n.item()) == nw
            assert np.array_equal(area.cpu().numpy()[1:nw + 1], np.bincount(want.ravel())[1:])


def test_cli_end_to_end(tmp_path, golden):
    from srcfinder_amd import cli_filtdet, detections, envi
    img, nodata = golden["a_ch4mf"], golden["a_nodata"]
    H, W = img.shape
    meta = {"lines": H, "samples": W, "bands": 4, "map info": "{ %s }" % ", ".join(str(v) for v in golden["mapinfo"])}
    path = str(tmp_path / "ang20200101t000000_cmf_img")
    mm = envi.create_image(path, meta, np.float64, "bip")
    mm[..., :3] = np.where(nodata[..., None], -9999.0, 1.0)
    mm[..., 3] = img
    mm.flush()
    del mm
    p = golden_params(golden, "a")
    out = tmp_path / "out"
    rc = cli_filtdet.main([path, str(out), "--kernel", str(p["k"]), "--mfmin", "500", "--mfmax", "1500", "--minarea", "9",
                           "--mfminsmall", "1250"])
    assert rc == 0
    stem = "ang20200101t000000_cmf_img"
    comp, _ = envi.open_memmap(str(out / (stem + "_ccomp")))
    want = golden["a_detcomp"].copy()
    want[nodata] = -9999
    assert np.array_equal(np.asarray(comp[0]), want)
    det, _ = envi.open_memmap(str(out / (stem + "_det")))
    wdet = np.where(img >= 500, img, 0.0)
    wdet[nodata] = -9999
    assert np.array_equal(np.asarray(det[0]), wdet)
    kde, kmeta = envi.open_memmap(str(out / (stem + "_kde")))
    wkde = np.clip((prestage(img, p["k"], False, False) - 500) / 1000.0, 0, 1)
    assert np.allclose(np.asarray(kde[0]), wkde, rtol=1e-12, atol=1e-300)
    assert "map info" in kmeta
    rows = (out / (stem + "_plumes.csv")).read_text().strip().splitlines()
    assert rows[0].split(",")[:3] == ["plumeid", "lid", "npix"]
    assert len(rows) - 1 == golden["a_detcomp"].max()
    ime = [float(r.split(",")[-1]) for r in rows[1:]]
    assert np.allclose(ime, golden["a_table_f"][:, 2], rtol=1e-12, atol=0)
    mi = detections.mapinfo(list(golden["mapinfo"]))
    assert float(mi["xps"]) == float(golden["ps"])


def test_detect_plumes_on_a_product(golden):
    import torch
    from srcfinder_amd import plumes
    img, nodata = golden["b_ch4mf"], golden["b_nodata"]
    prod = np.ones(img.shape + (4,))
    prod[..., 3] = img
    prod[nodata, :3] = -9999.0
    kde, comp, (header, rows) = plumes.detect_plumes(torch.as_tensor(prod).cuda(), list(golden["mapinfo"]), lid="x",
                                                      **golden_params(golden, "b"))
    assert np.array_equal(comp.cpu().numpy(), golden["b_detcomp"])
    assert [r[0] for r in rows] == ["x-%d" % (i + 1) for i in range(len(rows))]
    assert np.allclose([r[-1] for r in rows], golden["b_table_f"][:, 2], rtol=1e-12, atol=0)

#!/usr/bin/env python3
"""Golden vectors for the CMF-threshold plume detector, produced by EXECUTING the reference's ``filtdet``, ``kde``,
``ime`` and ``ime_scale`` (srcfinder_util.py:1383-1387, :1422-1482, :1989-1996).

Only runs in the development container (needs /root/reference).  ``srcfinder_util`` is imported unmodified; the
third-party functions this image lacks are served by stand-ins written from their published definitions:

* ``skimage.measure.label`` (``imlabel``, connectivity 2) -> ``scipy.ndimage.label`` with the 3 x 3 structure (same raster
  numbering);
* ``skimage.morphology.remove_small_objects`` on a boolean image -> ``scipy.ndimage.label`` with the cross (connectivity
  1, skimage's default), ``bincount`` of the labels, components of size ``< min_size`` cleared;
* ``skimage.segmentation.relabel_sequential`` -> the sorted non-zero labels mapped to 1..n (returns the relabelled image,
  the forward and the inverse map);
* ``skimage.morphology.reconstruction``: imported at the top of ``filtdet`` and used only under ``if 0:``, a stub;
* ``np.bool8`` (removed in numpy 2) -> ``np.bool_``; the file readers / writers, GDAL, rasterio, geopandas, spectral and
  the UTM module are stubs (no output file is asked of ``filtdet``).

Per scene the file keeps the inputs (half-integer ppm m, stored as int16 of twice the value; read them as float64 / 2), the parameters, ``filtdet``'s (detkde, detcomp) and the plume table: per component npix, bounding slices,
max and its first (row, col) in raster order, sum, and ``ime(pixels, ps)`` from the reference.  The generator asserts a
margin: no pixel's pre-clip value lies within 1e-9 relative of ``mfmin``, so a rounding difference in the blur cannot
flip a pixel and label maps compare exactly.  It also asserts that each scene exercises what it is for (4- vs
8-connectivity changes the outcome, the restore step restores, the ~ch4min compaction drops labels).

    python tests/golden/gen_golden_filtdet.py
"""
import os
import sys
import types
import warnings

import numpy as np
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
# ulx / uly / pixel size / zone / rotation of the reference's sample CMF product header (as gen_golden_detections.py)
MAPINFO = ["UTM", "1", "1", "272247.152557", "3992010.65018", "3.1", "3.1", "11", "North", "WGS-84", "units=Meters",
           "rotation=17.0000000"]
PS = 3.1


def _stub(name, **a):
    m = types.ModuleType(name)
    m.__dict__.update(a)
    sys.modules[name] = m
    return m


def _label(a, connectivity=None, **k):
    return ndi.label(a, structure=ndi.generate_binary_structure(a.ndim, connectivity or a.ndim))[0]


def _remove_small_objects(ar, min_size=64, connectivity=1, in_place=False, out=None):
    out = ar.copy() if out is None else out
    ccs = ndi.label(ar, structure=ndi.generate_binary_structure(ar.ndim, connectivity))[0]
    too_small = np.bincount(ccs.ravel()) < min_size
    out[too_small[ccs]] = 0
    return out


def _relabel_sequential(lab, offset=1):
    u = np.unique(lab)
    u = u[u != 0]
    fwd = np.zeros(int(lab.max()) + 1 if lab.size else 1, dtype=lab.dtype)
    fwd[u] = np.arange(offset, offset + len(u))
    return fwd[lab], fwd, np.concatenate([[0], u])


def load_reference():
    for name in ("gdal", "rasterio", "geopandas", "spectral", "spectral.io", "skimage"):
        _stub(name)
    _stub("osgeo", gdal=sys.modules["gdal"])
    sys.modules["gdal"].gdalconst = sys.modules["gdal"].ogr = sys.modules["gdal"].osr = None
    _stub("spectral.io.envi", open=lambda *a, **k: None)
    sys.modules["spectral"].SpyFile = type("SpyFile", (), {})
    _stub("LatLongUTMconversion", UTMtoLL=None, LLtoUTM=None)
    sys.modules["skimage"].__path__ = []
    _stub("skimage.measure", label=_label)
    _stub("skimage.morphology", remove_small_objects=_remove_small_objects, reconstruction=None,
          disk=lambda r, **k: np.ones((2 * r + 1, 2 * r + 1), bool))     # a default argument evaluated at import
    _stub("skimage.segmentation", relabel_sequential=_relabel_sequential)
    if not hasattr(np, "bool8"):
        np.bool8 = np.bool_
    sys.path.insert(0, REF)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import srcfinder_util as U
    return U


def _blobs(rng, img, n, amp, rmin, rmax, margin=6):
    H, W = img.shape
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(n):
        cy, cx = rng.integers(margin, H - margin), rng.integers(margin, W - margin)
        ry, rx = rng.uniform(rmin, rmax), rng.uniform(rmin, rmax)
        a = amp[0] + (amp[1] - amp[0]) * rng.random()
        q = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        img += np.where(q < 9.0, a * np.exp(-q), 0.0)          # truncated at 3 radii


def _structures(img, y, x, vdiag_weak=900.0, vdiag_strong=1400.0, vsmall_strong=1600.0, vsmall_weak=900.0):
    """Diagonal staircases (4-connected: single pixels; 8-connected: one component of 12) -- one weak, one with a strong
    pixel -- and 2 x 2 blobs, one strong, one weak."""
    for k in range(12):
        img[y + k, x + k] = vdiag_weak
        img[y + k, x + 20 + k] = vdiag_strong if k == 5 else vdiag_weak
    img[y + 3:y + 5, x + 40:x + 42] = vsmall_strong
    img[y + 8:y + 10, x + 40:x + 42] = vsmall_weak


def scene(name):
    """(ch4mf [H, W] float64 with NODATA, nodata [H, W] bool, params)."""
    if name == "a":
        rng = np.random.default_rng(11)
        H, W = 180, 90
        img = rng.normal(0.0, 2.0, (H, W))
        _blobs(rng, img, 10, (900, 2500), 2.0, 6.0)
        _structures(img, 120, 10)
        params = dict(minarea=9, mfmin=500, mfmax=1500, k=5, mfminsmall=1250, skip_kde=False, use_abs=False)
    elif name == "b":
        rng = np.random.default_rng(12)
        H, W = 400, 300
        img = rng.normal(0.0, 2.0, (H, W))
        _blobs(rng, img, 25, (900, 3000), 2.0, 12.0)
        _structures(img, 300, 100)
        params = dict(minarea=9, mfmin=500, mfmax=1500, k=50, mfminsmall=1250, skip_kde=False, use_abs=False)
    elif name == "c":
        rng = np.random.default_rng(13)
        H, W = 180, 90
        img = rng.normal(0.0, 2.0, (H, W))
        # |NODATA| = 9999 dominates the normalisation with use_abs: strong, wide enhancements of both signs
        _blobs(rng, img, 8, (4000, 8000), 3.0, 8.0)
        neg = np.zeros((H, W))
        _blobs(rng, neg, 8, (4000, 8000), 3.0, 8.0)
        img -= neg
        params = dict(minarea=9, mfmin=500, mfmax=1500, k=5, mfminsmall=1250, skip_kde=False, use_abs=True)
    elif name == "d":
        rng = np.random.default_rng(14)
        H, W = 180, 90
        img = rng.normal(0.0, 2.0, (H, W))
        _blobs(rng, img, 10, (900, 2500), 2.0, 6.0)
        _structures(img, 120, 10)
        params = dict(minarea=9, mfmin=500, mfmax=1500, k=50, mfminsmall=1250, skip_kde=True, use_abs=False)
    elif name == "e":
        rng = np.random.default_rng(15)
        H, W = 180, 90
        img = rng.normal(0.0, 2.0, (H, W))
        _blobs(rng, img, 10, (900, 2500), 2.0, 6.0)
        _structures(img, 120, 10)
        params = dict(minarea=9, mfmin=500, mfmax=1500, k=5, mfminsmall=400, skip_kde=False, use_abs=False)
    elif name == "f":            # the blur radius (50) exceeds both sides: scipy's reflection repeats
        rng = np.random.default_rng(16)
        H, W = 70, 40
        img = rng.normal(0.0, 2.0, (H, W))
        _blobs(rng, img, 5, (1200, 3000), 2.0, 5.0, margin=4)
        params = dict(minarea=9, mfmin=500, mfmax=1500, k=50, mfminsmall=1250, skip_kde=False, use_abs=False)
    else:
        raise KeyError(name)
    nodata = np.zeros((H, W), bool)
    nodata[:4, :] = True                       # a NODATA border, as the product carries it (RGB band 0 == -9999)
    nodata[:, -3:] = True
    img = np.floor(img) + 0.5                  # half-integer ppm m: never on an integer threshold, stored exactly as int16
    img[nodata] = -9999.0
    return img, nodata, params


def _int16(img):
    """2 x the plane as int16 (exact: the values are half-integers or -9999)."""
    assert np.array_equal(2 * img, np.round(2 * img)) and np.abs(2 * img).max() < 32768
    return (2 * img).astype(np.int16)


def prestage(U, img, p):
    d = np.abs(img) if p["use_abs"] else img.copy()
    return d if p["skip_kde"] else U.kde(d, k=p["k"])


def table(U, img, detcomp):
    rows, imes = [], []
    for i in range(1, int(detcomp.max()) + 1):
        m = detcomp == i
        ys, xs = np.nonzero(m)
        vals = img[m]
        j = int(np.argmax(vals))
        rows.append([m.sum(), ys.min(), ys.max() + 1, xs.min(), xs.max() + 1, ys[j], xs[j]])
        imes.append([vals.sum(), vals.max(), U.ime(vals, PS)])
    return np.array(rows, np.int64).reshape(-1, 7), np.array(imes, np.float64).reshape(-1, 3)


def main():
    U = load_reference()
    # filtdet only formats the map info for its (unused) writers: the package's parser of the header list serves
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from srcfinder_amd.detections import mapinfo
    mi = mapinfo(list(MAPINFO))
    out = {"mapinfo": np.array(MAPINFO), "ps": PS, "ime_scale_ps": U.ime_scale(PS), "scenes": np.array(list("abcdef"))}
    for name in "abcdef":
        img, nodata, p = scene(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            detkde, detcomp = U.filtdet(img.copy(), nodata, dict(mi), **p)
            pre = prestage(U, img, p)
        rel = np.abs(pre - p["mfmin"]) / p["mfmin"]
        assert rel.min() > 1e-9, "scene %s: a pre-clip value lies within 1e-9 of mfmin (%g)" % (name, rel.min())
        # what the scene is for
        clip = np.clip((pre - p["mfmin"]) / (p["mfmax"] - p["mfmin"]), 0, 1) > 0
        kept4 = _remove_small_objects(clip, p["minarea"], connectivity=1)
        kept8 = _remove_small_objects(clip, p["minarea"], connectivity=2)
        if name in "ad":
            assert not np.array_equal(kept4, kept8), "scene %s: 4- and 8-connectivity agree" % name
        if name in "abd":
            assert (clip & ~kept4).any() and (img[(clip & ~kept4)] >= p["mfminsmall"]).any(), name
        if name == "c":
            assert 0 < int(detcomp.max()) < int(_label(kept4).max()), "scene c: the compaction drops no label"
        rows, vals = table(U, img, detcomp)
        out.update({"%s_ch4mf" % name: _int16(img), "%s_nodata" % name: nodata, "%s_detkde" % name: detkde, "%s_detcomp" % name: detcomp.astype(np.int32),
                    "%s_table_int" % name: rows, "%s_table_f" % name: vals,
                    "%s_params" % name: np.array([p["minarea"], p["mfmin"], p["mfmax"], p["k"], p["mfminsmall"],
                                                  p["skip_kde"], p["use_abs"]], np.float64)})
        print("scene %s: %s -> %d plumes, %d pixels, min margin %.2e" % (name, img.shape, detcomp.max(), (detcomp > 0).sum(),
                                                                          rel.min()))
    import scipy
    out["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__])
    np.savez_compressed(os.path.join(HERE, "filtdet_golden.npz"), **out)


if __name__ == "__main__":
    main()

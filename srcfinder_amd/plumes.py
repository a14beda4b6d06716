"""CMF-threshold plume detector and per-plume IME on MI355X (the reference's CNN-free detection route).

Mirrors ``srcfinder_util.filtdet`` (:1422-1482) with its ``kde`` (:1383-1387): a Gaussian "KDE" weighting of the CMF
image, the ``mfmin`` .. ``mfmax`` ppm m threshold band, removal of components of fewer than ``minarea`` pixels
(skimage's ``remove_small_objects``: 4-connected, ``size < min_size``), the restoration of small components that hold a
pixel of at least ``mfminsmall``, and the final 8-connected labelling with the ``~ch4min`` pixels dropped and the labels
renumbered in order (``relabel_sequential``).  ``plume_table`` adds per component the pixel count, bounding slices, the
maximum and its first (row, col), the sum and the integrated mass enhancement ``ime = sum * ime_scale(ps)``
(:1989-1996).  Every stage runs in ``csrc/plumes.hip`` (and the labelling of ``csrc/masks.hip``); there is no CPU path.
The emission rate is not computed: the reference takes its IME-over-fetch input from outside.
"""
from __future__ import annotations

import math

import numpy as np

from . import _ffi

# srcfinder_util.py:106-109
KERNEL, MFMIN, MFMAX, MINAREA, MFMINSMALL = 50, 500, 1500, 9, 1250
MAX_RADIUS = 192        # sf_plumes_gauss_pass: the column tile of the blur holds 256 + 2 radius rows in LDS
NODATA = -9999

HEADER = ["plumeid", "lid", "npix", "bbminr", "bbmaxr", "bbminc", "bbmaxc",
          "ppmmmax", "ppmmmaxrow", "ppmmmaxcol", "ppmmmaxlat", "ppmmmaxlon", "ppmmsum", "ime_kg"]
# plume_table(..., saliency=): the CNN saliency per plume, named as in the reference's detection table (salience_predictions.py:32)
SALIENCY_COLUMNS = ["salmax", "salmaxrow", "salmaxcol"]


def ime_scale(ps):
    """``srcfinder_util.ime_scale`` (:1989-1992): kg per ppm m summed over pixels of ``ps`` m (ppm m -> m^3 per pixel
    area -> L -> mol at 22.4 L/mol -> kg at 0.01604 kg/mol)."""
    return (1.0 / 1e6) * ((ps * ps) / 1.0) * (1000.0 / 1.0) * (1.0 / 22.4) * (0.01604 / 1.0)


def ime(pixels_ppmm, ps):
    """``srcfinder_util.ime`` (:1994-1996): the integrated mass enhancement in kg of a set of ppm m pixels."""
    pixels_ppmm = np.asarray(pixels_ppmm)
    if not (np.isfinite(pixels_ppmm) & (pixels_ppmm >= 0)).all():
        raise ValueError("ime: pixel values must be finite and non-negative")
    return pixels_ppmm.sum() * ime_scale(ps)


def gaussian_weights(sigma, truncate=1.0):
    """scipy.ndimage's ``_gaussian_kernel1d(sigma, 0, radius)`` with ``radius = int(truncate * sigma + 0.5)``."""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum(), radius


def _check_args(shape, minarea, mfmin, mfmax, k, skip_kde):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("ch4mf must be a non-empty 2-d [lines, samples] plane, got shape %s" % (tuple(shape),))
    if not mfmax > mfmin:
        raise ValueError("mfmax (%r) must exceed mfmin (%r)" % (mfmax, mfmin))
    if mfmin <= 0:
        raise ValueError("mfmin must be positive (components are pixels of ch4mf >= mfmin), got %r" % (mfmin,))
    if int(minarea) != minarea or minarea < 0:
        raise ValueError("minarea must be a non-negative integer, got %r" % (minarea,))
    if not skip_kde:
        if not (k > 0 and math.isfinite(k)):
            raise ValueError("kernel sigma k must be positive, got %r" % (k,))
        if int(k + 0.5) > MAX_RADIUS:
            raise ValueError("kernel sigma k=%r gives a blur radius above %d" % (k, MAX_RADIUS))


def _to_device(a, dtype):
    import torch
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    t = t if t.is_cuda else t.cuda()
    return t.to(dtype).contiguous()


def filtdet(ch4mf, nodata_mask, minarea=MINAREA, mfmin=MFMIN, mfmax=MFMAX, k=KERNEL, mfminsmall=MFMINSMALL, skip_kde=False,
            use_abs=False, return_kde=False):
    """``filtdet`` of the reference for a [H, W] CMF plane (NODATA included, as the reference blurs it) and its
    [H, W] boolean nodata mask.  Returns ``(detkde float64, detcomp int32)`` torch tensors on the device: the clipped
    KDE weighting zeroed outside ``ch4mf >= mfmin`` and on nodata, and the components 1..n.  ``return_kde=True`` adds the
    clipped weighting before that zeroing (the reference's ``kde_outf`` image) as a third tensor."""
    import torch
    if not torch.cuda.is_available():
        raise _ffi.SrcfinderError("no GPU visible: srcfinder_amd has no CPU fallback")
    shape = tuple(ch4mf.shape)
    _check_args(shape, minarea, mfmin, mfmax, k, skip_kde)
    if tuple(nodata_mask.shape) != shape:
        raise ValueError("nodata_mask shape %s differs from ch4mf %s" % (tuple(nodata_mask.shape), shape))
    x = _to_device(ch4mf, torch.float64)
    H, W = shape
    dev = x.device
    L = _ffi.lib()
    P, st = _ffi.ptr, _ffi.stream_ptr
    with torch.cuda.device(dev):
        nod = _to_device(nodata_mask, torch.bool).to(torch.uint8)
        g = mm = None
        if not skip_kde:
            w, radius = gaussian_weights(k)
            wd = torch.as_tensor(w, dtype=torch.float64, device=dev)
            tmp = torch.empty((H, W), dtype=torch.float64, device=dev)
            g = torch.empty((H, W), dtype=torch.float64, device=dev)
            mm = torch.empty(2, dtype=torch.float64, device=dev)
            gs = torch.empty(max(L.sf_plumes_gauss_scratch_bytes(H, W), 1), dtype=torch.uint8, device=dev)
            # gaussian_filter: axis 0, then axis 1 (with the global min / max of the result reduced on the device)
            _ffi.check(L.sf_plumes_gauss_pass(P(x), P(tmp), H, W, 0, P(wd), radius, int(bool(use_abs)), None, None, st()),
                       "sf_plumes_gauss_pass")
            _ffi.check(L.sf_plumes_gauss_pass(P(tmp), P(g), H, W, 1, P(wd), radius, 0, P(mm), P(gs), st()),
                       "sf_plumes_gauss_pass")
            del tmp
        detkde = torch.empty((H, W), dtype=torch.float64, device=dev)
        ch4min = torch.empty((H, W), dtype=torch.uint8, device=dev)
        detmask = torch.empty((H, W), dtype=torch.uint8, device=dev)
        _ffi.check(L.sf_plumes_threshold(P(x), P(g), P(mm), H, W, float(mfmin), float(mfmax), int(bool(use_abs)), P(detkde),
                                         P(ch4min), P(detmask), st()), "sf_plumes_threshold")
        del g
        kde_raw = detkde.clone() if return_kde else None
        detsmall = detmask.clone()
        labels = torch.empty((H, W), dtype=torch.int32, device=dev)
        ncomp = torch.empty(1, dtype=torch.int32, device=dev)
        lscratch = torch.empty(L.sf_image_label8_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
        # remove_small_objects: 4-connected, components of fewer than minarea pixels go (:1453)
        area_cap = ((H + 1) // 2) * W + 2          # 4-connected components of an H x W mask: at most ceil(H/2) * W
        area = torch.empty(area_cap, dtype=torch.int32, device=dev)
        _ffi.check(L.sf_image_label4(P(detmask), H, W, P(labels), P(area), area_cap, P(ncomp), P(lscratch), st()),
                   "sf_image_label4")
        _ffi.check(L.sf_image_filter_small_components(P(labels), P(area), int(minarea), P(detmask), H, W, st()),
                   "sf_image_filter_small_components")
        del area
        if mfminsmall >= mfmin:                                                          # :1455-1463
            rs = torch.empty(L.sf_plumes_restore_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
            _ffi.check(L.sf_plumes_restore_small(P(detsmall), P(detmask), P(x), float(mfminsmall), H, W, P(rs), st()),
                       "sf_plumes_restore_small")
            del rs
        del detsmall
        _ffi.check(L.sf_image_label8(P(detmask), H, W, P(labels), None, 0, P(ncomp), P(lscratch), st()), "sf_image_label8")
        cs = torch.empty(L.sf_plumes_compact_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
        _ffi.check(L.sf_plumes_compact(P(labels), P(ncomp), P(ch4min), P(nod), P(detkde), H, W, P(cs), st()),
                   "sf_plumes_compact")
    if return_kde:
        return detkde, labels, kde_raw
    return detkde, labels


def plume_table(ch4mf, detcomp, mapinfo=None, lid="", as_dataframe=False, saliency=None):
    """Per component 1..n of ``detcomp``: npix, bounding slices (row start, row stop, col start, col stop), the max ppm m
    with its first (row, col) in raster order and their lat/lon (``detections.sl2latlon``; NaN without ``mapinfo``),
    the sum of ppm m and ``ime_kg = sum * ime_scale(ps)`` with ``ps`` the map info's pixel size (``xps``; NaN without).
    ``mapinfo``: a dict from ``detections.mapinfo`` or the header's ``map info``.  ``saliency``: an optional [H, W] CNN
    saliency map (e.g. ``cnn.predict_flightline(..., mask=detcomp > 0)``); each row then ends with ``salmax``, ``salmaxrow``,
    ``salmaxcol`` -- the largest saliency over the component's pixels that are not -9999 and its first (row, col) in raster
    order (NaN, -1, -1 when it has none).  Returns ``(header, rows)`` (header = HEADER, + SALIENCY_COLUMNS with ``saliency``)
    or a DataFrame."""
    import torch
    from . import detections
    if not torch.cuda.is_available():
        raise _ffi.SrcfinderError("no GPU visible: srcfinder_amd has no CPU fallback")
    if tuple(ch4mf.shape) != tuple(detcomp.shape) or len(ch4mf.shape) != 2:
        raise ValueError("ch4mf %s and detcomp %s must be the same 2-d shape" % (tuple(ch4mf.shape), tuple(detcomp.shape)))
    if mapinfo is not None and not isinstance(mapinfo, dict):
        mapinfo = detections.mapinfo(mapinfo)
    if saliency is not None and tuple(saliency.shape) != tuple(detcomp.shape):
        raise ValueError("saliency %s and detcomp %s must be the same shape" % (tuple(saliency.shape), tuple(detcomp.shape)))
    x = _to_device(ch4mf, torch.float64)
    lab = _to_device(detcomp, torch.int32)
    H, W = x.shape
    L = _ffi.lib()
    P, st = _ffi.ptr, _ffi.stream_ptr
    with torch.cuda.device(x.device):
        n = int(lab.max().item()) if lab.numel() else 0
        irec = torch.empty((n + 1, 8), dtype=torch.int32, device=x.device)
        drec = torch.zeros((n + 1, 2), dtype=torch.float64, device=x.device)
        _ffi.check(L.sf_plumes_stats(P(lab), P(x), H, W, n, P(irec), P(drec), st()), "sf_plumes_stats")
        if saliency is not None:
            sal = _to_device(saliency, torch.float32).to(x.device)
            smax = torch.empty(n + 1, dtype=torch.float32, device=x.device)
            sidx = torch.empty(n + 1, dtype=torch.int32, device=x.device)
            _ffi.check(L.sf_plumes_saliency(P(lab), P(sal), H, W, n, P(irec), P(smax), P(sidx), st()), "sf_plumes_saliency")
            smax, sidx = smax.cpu().numpy()[1:], sidx.cpu().numpy()[1:]
        irec = irec.cpu().numpy()[1:]
        drec = drec.cpu().numpy()[1:]
    ps = float(mapinfo["xps"]) if mapinfo is not None and mapinfo.get("xps") is not None else float("nan")
    scale = ime_scale(ps)
    rows = []
    for i in range(n):
        npix, r0, r1, c0, c1, mr, mc, _ = (int(v) for v in irec[i])
        if npix == 0:                     # a label absent from the plane (detcomp not from filtdet): nothing to report
            continue
        lat = lon = float("nan")
        if mapinfo is not None and mapinfo.get("proj"):
            ll = detections.sl2latlon(mc, mr, mapinfo)
            if ll is not None:
                lat, lon = (float(np.asarray(v).reshape(-1)[0]) for v in ll)
        s, m = float(drec[i, 0]), float(drec[i, 1])
        rows.append(["%s-%d" % (lid, i + 1) if lid else str(i + 1), lid, npix, r0, r1, c0, c1, m, mr, mc, lat, lon, s,
                     s * scale])
        if saliency is not None:
            k = int(sidx[i])
            rows[-1] += [float(smax[i]), k // W if k >= 0 else -1, k % W if k >= 0 else -1]
    header = HEADER + SALIENCY_COLUMNS if saliency is not None else HEADER
    if not as_dataframe:
        return header, rows
    from pandas import DataFrame
    return DataFrame.from_records(rows, columns=header)


def detect_plumes(product_out, mapinfo=None, lid="", **kw):
    """``filtdet`` + ``plume_table`` on a [H, W, 4] matched-filter product (band 3 = CMF; nodata where RGB band 0 is
    -9999, as ``detections`` reads it).  Returns ``(detkde, detcomp, (HEADER, rows))``."""
    import torch
    if not torch.cuda.is_available():
        raise _ffi.SrcfinderError("no GPU visible: srcfinder_amd has no CPU fallback")
    if len(product_out.shape) != 3 or product_out.shape[2] != 4:
        raise ValueError("product_out must be [H, W, 4] (R, G, B, CMF), got %s" % (tuple(product_out.shape),))
    prod = _to_device(product_out, torch.float64)
    cmf = prod[..., 3].contiguous()
    nodata = prod[..., 0] == NODATA
    detkde, detcomp = filtdet(cmf, nodata, **kw)
    return detkde, detcomp, plume_table(cmf, detcomp, mapinfo, lid=lid)

#!/usr/bin/env python3
"""Plume detector benchmark: one JSON line of per-stage and total ms for filtdet + the plume table on a synthetic
598-sample x 20000-line CMF plane (srcfinder_amd.synth.make_cmf_plane), the Gaussian passes' achieved GB/s (each pass
reads and writes the 95.7 MB float64 plane once) against the 8 TB/s HBM peak, and the scipy / numpy time of the same
work on the host for context.
   python tools/bench_filtdet.py [--lines 20000] [--samples 598] [--reps 20] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def cpu_filtdet(img, nodata, k=50, mfmin=500, mfmax=1500, minarea=9, mfminsmall=1250):
    """The rules of srcfinder_util.filtdet with scipy / numpy (skimage's label, remove_small_objects, relabel_sequential
    stated with scipy.ndimage), timed per stage."""
    import scipy.ndimage as ndi
    t = {}
    t0 = time.perf_counter()
    g = ndi.gaussian_filter(img, sigma=k, truncate=1)
    t["gauss"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    d = img * ((g - g.min()) / (g.max() - g.min()))
    d = np.clip((d - mfmin) / (mfmax - mfmin), 0, 1)
    ch4min, m = img >= mfmin, d > 0
    t["threshold"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lab = ndi.label(m)[0]
    kept = m & (np.bincount(lab.ravel())[lab] >= minarea)
    small = ndi.label(m & ~kept, structure=np.ones((3, 3)))[0]
    kept |= np.isin(small, np.unique(small[(img >= mfminsmall) & (small > 0)])) & (small > 0)
    comp = ndi.label(kept, structure=np.ones((3, 3)))[0]
    comp[~ch4min] = 0
    u = np.unique(comp[comp > 0])
    fwd = np.zeros(comp.max() + 1, np.int32)
    fwd[u] = np.arange(1, len(u) + 1)
    comp = fwd[comp]
    comp[nodata] = 0
    d[~ch4min] = 0
    d[nodata] = 0
    t["label"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    objs = ndi.find_objects(comp)
    for i, sl in enumerate(objs):
        v = img[sl][comp[sl] == i + 1]
        v.sum(), v.max()
    t["table"] = time.perf_counter() - t0
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20000)
    ap.add_argument("--samples", type=int, default=598)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from srcfinder_amd import _ffi, plumes
    from srcfinder_amd.synth import make_cmf_plane
    H, W = args.lines, args.samples
    img = make_cmf_plane(H, W, seed=2026)
    x = torch.as_tensor(img).cuda()
    nod = (x == -9999)
    L, P, st = _ffi.lib(), _ffi.ptr, _ffi.stream_ptr
    w, radius = plumes.gaussian_weights(plumes.KERNEL)
    wd = torch.as_tensor(w).cuda()
    tmp, g = torch.empty_like(x), torch.empty_like(x)
    mm = torch.empty(2, dtype=torch.float64, device="cuda")
    gs = torch.empty(L.sf_plumes_gauss_scratch_bytes(H, W), dtype=torch.uint8, device="cuda")
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        a, b = ev(), ev()
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps

    ms = {}
    ms["gauss_axis0"] = timed(lambda: _ffi.check(L.sf_plumes_gauss_pass(P(x), P(tmp), H, W, 0, P(wd), radius, 0, None, None,
                                                                        st()), "gauss0"))
    ms["gauss_axis1_minmax"] = timed(lambda: _ffi.check(L.sf_plumes_gauss_pass(P(tmp), P(g), H, W, 1, P(wd), radius, 0, P(mm),
                                                                               P(gs), st()), "gauss1"))
    detkde = torch.empty_like(x)
    ch4min = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    detmask = torch.empty_like(ch4min)
    ms["threshold"] = timed(lambda: _ffi.check(L.sf_plumes_threshold(P(x), P(g), P(mm), H, W, 500.0, 1500.0, 0, P(detkde),
                                                                      P(ch4min), P(detmask), st()), "threshold"))
    ms["filtdet_total"] = timed(lambda: plumes.filtdet(x, nod))
    ms["labelling_etc"] = ms["filtdet_total"] - ms["gauss_axis0"] - ms["gauss_axis1_minmax"] - ms["threshold"]
    kde, comp = plumes.filtdet(x, nod)
    n = int(comp.max().item())
    irec = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda")
    drec = torch.empty((n + 1, 2), dtype=torch.float64, device="cuda")
    ms["plume_stats"] = timed(lambda: _ffi.check(L.sf_plumes_stats(P(comp), P(x), H, W, n, P(irec), P(drec), st()), "stats"))
    t0 = time.perf_counter()
    for _ in range(3):
        plumes.plume_table(x, comp, {"xps": 5.0})
    ms["plume_table_py"] = (time.perf_counter() - t0) / 3 * 1e3
    ms["total"] = ms["filtdet_total"] + ms["plume_table_py"]
    plane_bytes = H * W * 8
    gbs = {k: 2 * plane_bytes / (ms[k] * 1e-3) / 1e9 for k in ("gauss_axis0", "gauss_axis1_minmax")}
    res = {"bench": "filtdet", "lines": H, "samples": W, "kernel": plumes.KERNEL, "radius": radius, "plumes": n,
           "ms": {k: round(v, 4) for k, v in ms.items()},
           "gauss_GBps": {k: round(v, 1) for k, v in gbs.items()},
           "gauss_frac_of_8TBps": {k: round(v * 1e9 / HBM_PEAK, 3) for k, v in gbs.items()},
           "device": torch.cuda.get_device_name(0)}
    if not args.no_cpu:
        t = cpu_filtdet(img, img == -9999)
        res["cpu_scipy_ms"] = {k: round(v * 1e3, 1) for k, v in t.items()}
        res["cpu_scipy_ms"]["total"] = round(sum(t.values()) * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

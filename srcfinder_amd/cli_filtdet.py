#!/usr/bin/env python3
"""Command line of the CMF-threshold plume detector (``srcfinder_util.filtdet``, :1422-1482, defaults :106-109):

    python -m srcfinder_amd.cli_filtdet CMF_IMG OUTDIR [--mfmin 500] [--mfmax 1500] [--minarea 9] [--kernel 50]
                                        [--mfminsmall 1250] [--use_abs] [--skip_kde] [--lid NAME]
                                        [--weights PT [--model COVID_QC] [--batch 1024]]

CMF_IMG is an ENVI matched-filter product (4 bands R, G, B, CMF; nodata where band 0 is -9999) or a single-band CMF
image (nodata where it is -9999).  OUTDIR receives the three images ``filtdet`` can write -- ``<stem>_kde`` (the clipped
KDE weighting before the ch4min / nodata zeroing; not with --skip_kde), ``<stem>_ccomp`` (components, -9999 on nodata)
and ``<stem>_det`` (ch4mf, 0 below mfmin, -9999 on nodata) -- and ``<stem>_plumes.csv``, the plume table with the
integrated mass enhancement of every component.  With ``--weights`` (a GoogLeNet state_dict) the CNN scores the windows
of the component pixels alone (``cnn.predict_flightline(mask=detcomp > 0)`` on the CMF band as float32): the table gains
``salmax``, ``salmaxrow``, ``salmaxcol`` and ``<stem>_saliency`` is written (float32; 0 outside the components, -9999 on
CNN NODATA).
"""
import argparse
import csv
import os
import os.path as op
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description="CMF-threshold plume detection (filtdet) with per-plume IME.")
    p.add_argument("cmf_img", help="ENVI CMF product (4 bands) or single-band CMF image")
    p.add_argument("outdir", help="output directory")
    p.add_argument("--mfmin", type=float, default=500.0, help="lower ppm m of the threshold band")
    p.add_argument("--mfmax", type=float, default=1500.0, help="upper ppm m of the threshold band")
    p.add_argument("--minarea", type=int, default=9, help="components of fewer pixels are removed (4-connected)")
    p.add_argument("--kernel", type=float, default=50.0, help="sigma of the KDE Gaussian (truncate=1)")
    p.add_argument("--mfminsmall", type=float, default=1250.0, help="small components with a pixel >= this are kept")
    p.add_argument("--use_abs", action="store_true", help="weight |ch4mf| instead of ch4mf")
    p.add_argument("--skip_kde", action="store_true", help="no KDE weighting")
    p.add_argument("--lid", default=None, help="line id of the plume ids (default: the image's stem)")
    p.add_argument("--weights", default=None, help="GoogLeNet state_dict (.pt): score the component pixels with the CNN")
    p.add_argument("--model", default="COVID_QC", choices=["COVID_QC", "CalCH4_v8", "Permian_QC", "multi_256", "multi_64"],
                   help="normalisation of the CNN's input (with --weights)")
    p.add_argument("--batch", type=int, default=1024, help="CNN windows per batch (with --weights)")
    return p


def _write(path, meta, arr, dtype):
    from . import envi
    m = {k: v for k, v in meta.items() if k in ("map info", "coordinate system string")}
    for k in m:                                     # read_header keeps these as the text between the braces
        if isinstance(m[k], str) and not m[k].lstrip().startswith("{"):
            m[k] = "{ %s }" % m[k]
    m.update(lines=arr.shape[0], samples=arr.shape[1], bands=1, **{"data ignore value": -9999})
    out = envi.create_image(path, m, dtype, "bsq")
    out[0] = arr
    out.flush()
    del out


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        print("[ERR] no GPU visible: srcfinder_amd has no CPU path, exiting.")
        return 1
    from . import detections, envi, plumes
    if args.weights is not None and not op.isfile(args.weights):
        print("[ERR] weights %s not found, exiting." % args.weights)
        return 1
    mm, meta = envi.open_memmap(args.cmf_img)
    bil = envi.to_bil(mm, meta)
    nb = bil.shape[1]
    if nb not in (1, 4):
        print("[ERR] %s has %d bands: expected a 4-band CMF product or a single-band CMF image" % (args.cmf_img, nb))
        return 1
    ch4mf = np.ascontiguousarray(bil[:, nb - 1, :], dtype=np.float64)
    nodata = np.asarray(bil[:, 0, :]) == -9999
    mi = detections.mapinfo(meta["map info"]) if "map info" in meta else None
    stem = op.splitext(op.basename(args.cmf_img))[0]
    lid = args.lid if args.lid is not None else stem
    os.makedirs(args.outdir, exist_ok=True)
    detkde, detcomp, kde_raw = plumes.filtdet(ch4mf, nodata, minarea=args.minarea, mfmin=args.mfmin, mfmax=args.mfmax,
                                              k=args.kernel, mfminsmall=args.mfminsmall, skip_kde=args.skip_kde,
                                              use_abs=args.use_abs, return_kde=True)
    sal = None
    if args.weights is not None:                                                    # the CNN on the component pixels alone
        from . import cnn
        sd = torch.load(args.weights, map_location="cpu")
        sal = cnn.predict_flightline(ch4mf.astype(np.float32), args.model, weights=sd, batch=args.batch, mask=detcomp > 0)
    header, rows = plumes.plume_table(ch4mf, detcomp, mi, lid=lid, saliency=sal)
    comp = detcomp.cpu().numpy()
    if not args.skip_kde:                                                           # kde_outf (:1438-1439)
        _write(op.join(args.outdir, stem + "_kde"), meta, kde_raw.cpu().numpy(), np.float64)
    ccomp = comp.copy()                                                             # ccomp_outf (:1469-1471)
    ccomp[nodata] = -9999
    _write(op.join(args.outdir, stem + "_ccomp"), meta, ccomp, np.int32)
    det = ch4mf.copy()                                                              # det_outf (:1478-1482)
    det[ch4mf < args.mfmin] = 0
    det[nodata] = -9999
    _write(op.join(args.outdir, stem + "_det"), meta, det, np.float64)
    if sal is not None:
        _write(op.join(args.outdir, stem + "_saliency"), meta, sal.cpu().numpy(), np.float32)
    with open(op.join(args.outdir, stem + "_plumes.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)
    ime = header.index("ime_kg")
    print("%d plumes, %.3f kg IME in all" % (len(rows), sum(r[ime] for r in rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())

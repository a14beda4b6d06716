#!/usr/bin/env python3
"""CNN scorer on pixel sets (sf_cnn_score_pixels: every masked window on its own, route split_unshared): one JSON line with
  * random masks of 0.1 %, 1 % and 10 % of a 2500 x 598 strip (synthetic_plane): windows/s and seconds of the scoring call
    (activation scales calibrated once beforehand; one warm-up call per mask);
  * the filtdet component pixels of a full synthetic flightline (synth.make_cmf_plane(20000, 598)): their count, the seconds of
    predict_flightline(mask=...) as a user calls it (plane preparation and calibration included) and the scoring call's windows/s;
  * the row route (sf_cnn_score_rows, shared trunk, two lanes) on 256 rows of the strip: where a mask stops paying off;
  * bit_identical: the masked values equal the row route's at every masked pixel of those 256 rows (and no batch was re-scored).
   python tools/bench_cnn_pixels.py [--batch 1024] [--case all|mask1|rows] [--row-route split|split_unshared] [--lanes N]
--case mask1 / rows: only the 1 % mask / only the row route, warm-up + one call (a process of its own for rocprofv3)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--case", default="all", choices=["all", "mask1", "rows"])
    ap.add_argument("--rows", type=int, default=256, help="image rows of the row-route reference")
    ap.add_argument("--row-route", default="split", help="route of the row reference (split: the shared trunk; split_unshared)")
    ap.add_argument("--lanes", type=int, default=None, help="row reference: concurrent row parts (default cnn.LANES; 1 for a per-launch profile)")
    args = ap.parse_args()
    import torch
    from srcfinder_amd import cnn, plumes, synth
    from srcfinder_amd.cnn_weights import synthetic_plane, synthetic_state_dict
    B = args.batch
    sd = synthetic_state_dict(2024)
    net = cnn.GoogLeNetHIP(sd)
    H, W = 2500, 598
    plane = synthetic_plane(H, W, seed=5)
    ds = cnn.FlightlineConvolve(plane, "COVID_QC")
    net.calibrate(ds, B)
    rng = np.random.default_rng(2026)
    split_unshared = cnn.ROUTES["split_unshared"]

    def timed(fn):
        fn()                                              # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    res = {"bench": "cnn_pixels", "strip": [H, W], "batch": B, "device": torch.cuda.get_device_name(0)}
    masked = {}
    fracs = {"mask1": [0.01]}.get(args.case, [0.001, 0.01, 0.1] if args.case == "all" else [])
    res["random_masks"] = []
    for f in fracs:
        pix = np.sort(rng.choice(H * W, int(round(f * H * W)), replace=False))
        pt = torch.as_tensor(pix, device="cuda")
        out = torch.zeros(H * W, dtype=torch.float32, device="cuda")
        dt, nres = timed(lambda: cnn._score_pixels_c(net, ds, pt, B, out, split_unshared))
        masked[f] = (pix, out, nres)
        res["random_masks"].append({"fraction": f, "windows": int(len(pix)), "s": round(dt, 4), "windows_per_s": round(len(pix) / dt, 1),
                                    "rescued_batches": nres})
    if args.case in ("all", "rows"):
        out_rows = torch.zeros(H * W, dtype=torch.float32, device="cuda")
        dt, nres = timed(lambda: cnn._score_rows_c(net, ds, 0, args.rows, B, out_rows, cnn.ROUTES[args.row_route],
                                                   args.lanes))
        res["row_route"] = {"route": args.row_route, "lanes": args.lanes or cnn.LANES, "rows": args.rows, "windows": args.rows * W, "s": round(dt, 4), "windows_per_s": round(args.rows * W / dt, 1),
                            "rescued_batches": nres}
        if masked:
            same, n = True, 0
            for pix, out, nr in masked.values():
                p = torch.as_tensor(pix[pix < args.rows * W], device="cuda")
                n += int(p.numel())
                same = same and nr == 0 and nres == 0 and torch.equal(out[p], out_rows[p])
            res["bit_identical"] = bool(same)
            res["bit_identical_pixels"] = n
    if args.case == "all":
        ch4mf = synth.make_cmf_plane(20000, 598)
        x = torch.as_tensor(ch4mf).cuda()
        _, comp = plumes.filtdet(x, x == -9999)
        m = comp > 0
        fl = ch4mf.astype(np.float32)
        info = {}
        dt, _ = timed(lambda: cnn.predict_flightline(fl, "COVID_QC", net=net, batch=B, mask=m, info=info))
        dsf = cnn.FlightlineConvolve(fl, "COVID_QC")
        net.calibrate(dsf, B)
        pt = torch.nonzero(m.reshape(-1)).reshape(-1)
        out = torch.zeros(20000 * 598, dtype=torch.float32, device="cuda")
        ds_, nres = timed(lambda: cnn._score_pixels_c(net, dsf, pt, B, out, split_unshared))
        res["flightline_candidates"] = {"shape": [20000, 598], "plumes": int(comp.max().item()), "pixels": int(pt.numel()),
                                        "fraction": round(pt.numel() / (20000 * 598), 5), "s_predict_flightline": round(dt, 3),
                                        "s_score": round(ds_, 3), "windows_per_s": round(pt.numel() / ds_, 1),
                                        "rescued_batches": info["rescued_batches"] + nres}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

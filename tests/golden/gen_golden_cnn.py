#!/usr/bin/env python3
"""Generate the CNN golden vectors with the REAL reference classes (development container only).

    python tests/golden/gen_golden_cnn.py            # cnn_googlenet_golden.npz
    python tests/golden/gen_golden_cnn.py --filled   # cnn_googlenet_filled_golden.npz: windows full of data

``cnn/archs/googlenet1.py`` imports as is (torch only).  ``cnn/cnn_pred_pipeline.py`` needs ``torchvision.transforms``
and ``rasterio`` (absent here): three trivial stand-in classes (Compose / Normalize / Pad) and a ``rasterio.open``
that returns the in-memory plane are placed in ``sys.modules``; ``ClampCH4`` and
``FlightlineConvolve`` then run unmodified.  The script's ``__main__`` needs a weights file next to the read-only
reference, so its 10-line batch loop (:173-189) is restated here around the imported classes.
Weights: ``srcfinder_amd.cnn_weights.synthetic_state_dict`` (trained ones are not in the checkout).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference"
from srcfinder_amd.cnn_weights import synthetic_plane, synthetic_state_dict  # noqa: E402

PLANE = {}


def install_stubs():
    tv, tr, rio = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("rasterio")

    class Compose:
        def __init__(s, ts): s.ts = ts
        def __call__(s, x):
            for t in s.ts:
                x = t(x)
            return x

    class Normalize:
        def __init__(s, mean, std):
            s.m, s.s = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)
        def __call__(s, x): return (x - s.m) / s.s

    class Pad:
        def __init__(s, padding, fill=0, padding_mode="constant"): s.p, s.fill = padding, fill
        def __call__(s, x):
            l, t, r, b = s.p
            return torch.nn.functional.pad(x, (l, r, t, b), value=s.fill)

    tr.Compose, tr.Normalize, tr.Pad = Compose, Normalize, Pad
    tv.transforms = tr
    rio.open = lambda path, *a, **k: types.SimpleNamespace(read=lambda band: PLANE[path])
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "rasterio": rio,
                        "matplotlib": types.ModuleType("matplotlib"),
                        "matplotlib.pyplot": types.ModuleType("matplotlib.pyplot")})
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    return Compose, Normalize


BLOCKS = ["conv1", "maxpool1", "conv2", "conv3", "maxpool2", "inception3a", "inception3b", "maxpool3",
          "inception4a", "inception4b", "inception4c", "inception4d", "inception4e", "maxpool4", "inception5a", "inception5b"]


def reference_model():
    """(cnn_pred_pipeline module, googlenet1 model with the seed-2024 weights, the COVID_QC transform)."""
    torch.set_num_threads(8)
    Compose, Normalize = install_stubs()
    sys.path.insert(0, os.path.join(REF, "cnn"))
    import cnn_pred_pipeline as P
    from archs.googlenet1 import googlenet

    sd_np = synthetic_state_dict(seed=2024)
    model = googlenet(pretrained=False, num_classes=2, init_weights=False).eval()
    full = model.state_dict()
    missing = [k for k in full if k not in sd_np and not k.startswith(("aux1.", "aux2.")) and not k.endswith("num_batches_tracked")]
    assert not missing, missing
    for k, v in sd_np.items():
        assert tuple(full[k].shape) == v.shape, k
        full[k] = torch.as_tensor(v)
    model.load_state_dict(full)

    mean, std = 110.6390, 183.9152          # COVID_QC, cnn_pred_pipeline.py:126-133
    tf = Compose([P.ClampCH4(vmin=0, vmax=4000), Normalize([mean], [std])])
    return P, model, tf


def main():
    P, model, tf = reference_model()

    # (1) FlightlineConvolve on a 40 x 30 plane with NODATA: padded image + three tiles
    plane = synthetic_plane(40, 30, seed=7)
    PLANE["p40"] = plane
    ds = P.FlightlineConvolve("p40", transform=tf)
    assert len(ds) == 40 * 30 and ds.dim == 256 and tuple(ds.inshape) == (1, 40, 30)
    tiles_idx = [0, 17 * 30 + 5, 40 * 30 - 1]
    out = dict(plane40=plane, padded40=ds.x.numpy(), tiles_idx=np.array(tiles_idx),
               tiles=np.stack([ds[i].numpy() for i in tiles_idx]))

    # (2) logits + per-block activation checksums for 6 tiles of that plane
    idx6 = [0, 31, 17 * 30 + 5, 600, 911, 1199]
    batch = torch.stack([ds[i] for i in idx6])
    acts = {}
    hooks = []
    for name in BLOCKS:
        hooks.append(getattr(model, name).register_forward_hook(lambda m, i, o, n=name: acts.__setitem__(n, o.detach())))
    with torch.no_grad():
        logits = model(batch)
    for h in hooks:
        h.remove()
    out["logits_idx"] = np.array(idx6)
    out["logits"] = logits.numpy()
    for n, a in acts.items():
        out["act_mean_" + n] = a.mean(dim=(0, 2, 3)).numpy()          # per-channel mean
        out["act_abs_" + n] = a.abs().mean().numpy()
    out["conv1_tile0_ch0"] = acts["conv1"][0, 0].numpy()               # one full 128x128 plane: pins padding/stride
    out["inception3a_tile0"] = acts["inception3a"][0, :, ::4, ::4].numpy()

    # (3) the batch loop of the script (:173-189) on a 24 x 20 plane
    plane2 = synthetic_plane(24, 20, seed=11)
    PLANE["p24"] = plane2
    ds2 = P.FlightlineConvolve("p24", transform=tf)
    loader = torch.utils.data.DataLoader(ds2, batch_size=32, shuffle=False, num_workers=0)
    allpred = []
    for b in loader:
        with torch.no_grad():
            preds = torch.nn.functional.softmax(model(b), dim=1)
            allpred += [x[1] for x in preds.cpu().detach().numpy()]
    allpred = np.array(allpred).reshape(plane2.shape)
    allpred[plane2 == -9999] = -9999
    out["plane24"] = plane2
    out["saliency24"] = allpred.astype(np.float32)
    out["versions"] = np.array("torch %s numpy %s" % (torch.__version__, np.__version__))
    np.savez_compressed(os.path.join(HERE, "cnn_googlenet_golden.npz"), **out)
    print("logits", logits.numpy())
    print("saliency range", allpred[allpred > -9999].min(), allpred.max())


# Windows full of data (the flightline case: > 98 % of a 598-column flightline's windows touch no plane edge).  Two planes,
# regenerated from (generator, shape, seed) at test time and pinned by a SHA-256 of their bytes:
#   A  synthetic_plane, 1400 x 300, with NODATA pixels inside the interior block.  Scored in one call at batch 512, the phase maps
#      are rebuilt every ~506 rows (SHARE_ROWS2 = 512) and, with the default two lanes, the second lane (rows 700..) rebuilds its
#      maps at row 1206: rows 1232..1239 are served by rebuilt maps, and they straddle a strip-map rebuild (STRIP_ROWS = 16) at
#      row 1235 with one lane and at 1237 with two.
#   B  synthetic_filled_plane, 320 x 300: data everywhere over the whole 0..4000 clamp, values outside it, NODATA pixels.
# Pinned per plane: an 8 x 8 block of consecutive interior windows (every phase of the 64-grid and 32-grid maps, >= 128 px from
# every edge), four windows that each hang over exactly one plane edge, the four corners, one interior NODATA pixel.
FILLED = {
    "A": dict(gen="synthetic_plane", H=1400, W=300, seed=41, block=(1232, 140), nodata=[(1234, 143), (1238, 146)]),
    "B": dict(gen="synthetic_filled_plane", H=320, W=300, seed=5, block=(148, 140), nodata=[]),
}


def filled_plane(key):
    from srcfinder_amd import cnn_weights
    c = FILLED[key]
    plane = getattr(cnn_weights, c["gen"])(c["H"], c["W"], seed=c["seed"])
    for r, q in c["nodata"]:
        plane[r, q] = -9999.0
    return plane


def filled_windows(key, plane):
    """(flat window indices, kind per window) of the pinned windows of plane `key`."""
    c = FILLED[key]
    H, W = plane.shape
    br, bc = c["block"]
    assert 128 <= br and br + 7 <= H - 129 and 128 <= bc and bc + 7 <= W - 129
    rc = [((br + i, bc + j), "block") for i in range(8) for j in range(8)]
    rc += [((3, W // 2), "edge_top"), ((H - 4, W // 2 + 5), "edge_bottom"), ((br + 3, 2), "edge_left"), ((br + 4, W - 3), "edge_right")]
    rc += [((0, 0), "corner"), ((0, W - 1), "corner"), ((H - 1, 0), "corner"), ((H - 1, W - 1), "corner")]
    blk = np.zeros(plane.shape, bool)
    blk[br:br + 8, bc:bc + 8] = True
    inner = np.zeros(plane.shape, bool)
    inner[128:H - 128, 128:W - 128] = True
    nod = np.argwhere((plane == -9999) & inner)
    assert len(nod), key
    if not any(blk[tuple(x)] for x in nod):                         # (else the block already holds one)
        rc.append((tuple(int(v) for v in nod[0]), "nodata"))
    idx = np.array([r * W + q for (r, q), _ in rc], np.int64)
    assert len(set(idx.tolist())) == len(idx)
    return idx, np.array([k for _, k in rc])


def main_filled():
    import hashlib
    P, model, tf = reference_model()
    out = {}
    for key in ("A", "B"):
        plane = filled_plane(key)
        name = "filled_" + key
        PLANE[name] = plane
        ds = P.FlightlineConvolve(name, transform=tf)
        idx, kind = filled_windows(key, plane)
        sums, count, logits = {}, 0, []
        hooks = [getattr(model, n).register_forward_hook(
            lambda m, i, o, n=n: sums.__setitem__(n, sums.get(n, 0) + o.detach().double().sum(dim=(0, 2, 3)) / (o.shape[2] * o.shape[3])))
            for n in BLOCKS]
        for a in range(0, len(idx), 16):                       # the script's loop (:173-189) over the pinned windows
            b = torch.stack([ds[int(i)] for i in idx[a:a + 16]])
            with torch.no_grad():
                logits.append(model(b))
            count += b.shape[0]
        for h in hooks:
            h.remove()
        logits = torch.cat(logits)
        prob = torch.nn.functional.softmax(logits, dim=1)[:, 1].numpy().astype(np.float32)
        prob[plane.reshape(-1)[idx] == -9999] = -9999
        c = FILLED[key]
        out.update({key + "_gen": np.array(c["gen"]), key + "_H": c["H"], key + "_W": c["W"], key + "_seed": c["seed"],
                    key + "_block": np.array(c["block"]), key + "_nodata": np.array(c["nodata"], np.int64).reshape(-1, 2),
                    key + "_sha256": np.array(hashlib.sha256(plane.tobytes()).hexdigest()),
                    key + "_idx": idx, key + "_kind": kind, key + "_logits": logits.numpy(), key + "_prob": prob})
        for n in BLOCKS:
            out[key + "_act_mean_" + n] = (sums[n] / count).float().numpy()   # per-channel mean over the pinned windows
        v = prob != -9999
        mid = (prob[v] > 1e-3) & (prob[v] < 1 - 1e-3)
        print(key, plane.shape, "windows", len(idx), "p range %.4g .. %.4g" % (prob[v].min(), prob[v].max()),
              "unsaturated %.1f %%" % (100 * mid.mean()), "mean |act| conv1 %.3g inception5b %.3g" % (
                  float(np.abs(out[key + "_act_mean_conv1"]).mean()), float(np.abs(out[key + "_act_mean_inception5b"]).mean())))
    out["versions"] = np.array("torch %s numpy %s" % (torch.__version__, np.__version__))
    np.savez_compressed(os.path.join(HERE, "cnn_googlenet_filled_golden.npz"), **out)


if __name__ == "__main__":
    main_filled() if "--filled" in sys.argv[1:] else main()

"""The CNN CPU oracle (oracle/cnn_oracle.py) against golden vectors produced by the REAL reference classes
(tests/golden/gen_golden_cnn.py).  Runs anywhere (torch CPU)."""
import os

import numpy as np
import pytest
import torch

from oracle import cnn_oracle as O
from srcfinder_amd import cnn_weights
from srcfinder_amd.cnn_weights import conv_table, synthetic_plane, synthetic_state_dict

MEAN, STD = O.MODEL_NORM["COVID_QC"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cnn_googlenet_golden.npz"))


@pytest.fixture(scope="module")
def sd():
    return synthetic_state_dict(seed=2024)


def test_weight_generator_is_stable(sd):
    # a pure integer hash: these values must never change (the goldens depend on them)
    assert len(conv_table()) == 57
    w = sd["conv1.conv.weight"]
    assert w.shape == (64, 1, 7, 7) and w.dtype == np.float32
    assert abs(float(w[0, 0, 0, 0]) - 0.10262156277894974) < 1e-9, float(w[0, 0, 0, 0])
    assert abs(float(sd["fc.bias"][1]) - (-0.009986969642341137)) < 1e-9, float(sd["fc.bias"][1])


def test_prepare_and_tiles(gold):
    plane = synthetic_plane(40, 30, seed=7)
    assert np.array_equal(plane, gold["plane40"])
    xpad = O.prepare_plane(plane, MEAN, STD)
    assert np.array_equal(xpad.numpy(), gold["padded40"])              # clamp/normalize/pad bit-exact
    for k, i in enumerate(gold["tiles_idx"]):
        assert np.array_equal(O.tile(xpad, int(i), 30).numpy(), gold["tiles"][k])
    # NODATA (-9999) becomes clamp -> 0 -> (0 - mean)/std; outside the image the pad is exactly 0
    assert xpad[0, 0, 0] == 0.0
    assert abs(float(xpad[0, 128, 128]) - (0.0 - MEAN) / STD) < 1e-6


def test_logits_and_activations(gold, sd):
    plane = gold["plane40"]
    xpad = O.prepare_plane(plane, MEAN, STD)
    b = torch.stack([O.tile(xpad, int(i), 30) for i in gold["logits_idx"]])
    taps = {}
    with torch.no_grad():
        logits = O.googlenet_forward(b, sd, taps).numpy()
    np.testing.assert_allclose(logits, gold["logits"], rtol=2e-5, atol=2e-5)
    for n, a in taps.items():
        np.testing.assert_allclose(a.mean(dim=(0, 2, 3)).numpy(), gold["act_mean_" + n], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(taps["conv1"][0, 0].numpy(), gold["conv1_tile0_ch0"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(taps["inception3a"][0, :, ::4, ::4].numpy(), gold["inception3a_tile0"], rtol=1e-4, atol=1e-5)


def test_predict_subset(gold, sd):
    plane = gold["plane24"]
    idx = [0, 1, 2, 19, 20, 12 * 20 + 6, 479]                     # includes NODATA pixels (0,0..2) and (12,6)
    got = O.predict_plane(plane, sd, MEAN, STD, indices=idx)
    want = gold["saliency24"].reshape(-1)[idx]
    assert np.array_equal(got == -9999, want == -9999)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6)


def test_fcn_shift_and_stitch_oracle_matches_reference(golden_dir, sd):
    """oracle.fcn_predict_plane against the golden of the reference's FlightlineShiftStitch / converted model /
    stitch_stack (tests/golden/gen_golden_fcn.py): same torch ops on the same machine class -> bit-identical stack
    and saliency map."""
    g = np.load(os.path.join(golden_dir, "cnn_fcn_golden.npz"))
    torch.set_num_threads(8)
    sal, stack = O.fcn_predict_plane(g["plane"], sd, float(g["mean"]), float(g["std"]), scale=int(g["scale"]))
    assert stack.shape == g["predstack"].shape
    np.testing.assert_allclose(stack, g["predstack"], rtol=1e-5, atol=1e-9)
    assert np.array_equal(sal == -9999, g["saliency"] == -9999)
    np.testing.assert_allclose(sal, g["saliency"], rtol=1e-5, atol=1e-9)


# --- windows full of data (tests/golden/gen_golden_cnn.py --filled): the flightline case the 40 x 30 / 24 x 20 planes above are not.
# There the windows are >= 98 % zero padding; here the activations are ~10x larger, enough for fp16-sized operand errors to show.

@pytest.fixture(scope="module")
def filled(golden_dir):
    return np.load(os.path.join(golden_dir, "cnn_googlenet_filled_golden.npz"))


def filled_plane(g, key):
    """Plane `key` of the filled golden, regenerated from its generator, shape and seed (+ its extra NODATA pixels)."""
    plane = getattr(cnn_weights, str(g[key + "_gen"]))(int(g[key + "_H"]), int(g[key + "_W"]), seed=int(g[key + "_seed"]))
    for r, c in g[key + "_nodata"]:
        plane[r, c] = -9999.0
    return plane


def _oracle_windows(plane, idx, sd, taps_sum=None):
    """logits of the windows `idx` of `plane` (the oracle, batches of 16); ``taps_sum``: per-block channel means, summed over windows."""
    xpad = O.prepare_plane(plane, MEAN, STD)
    out = []
    with torch.no_grad():
        for a in range(0, len(idx), 16):
            taps = {}
            b = torch.stack([O.tile(xpad, int(i), plane.shape[1]) for i in idx[a:a + 16]])
            out.append(O.googlenet_forward(b, sd, taps))
            if taps_sum is not None:
                for n, t in taps.items():
                    taps_sum[n] = taps_sum.get(n, 0) + t.double().mean(dim=(2, 3)).sum(0)
    return torch.cat(out)


def _prob(logits, plane, idx):
    p = torch.softmax(logits, dim=1)[:, 1].numpy().astype(np.float32)
    p[plane.reshape(-1)[idx] == -9999] = -9999
    return p


def test_filled_planes_reproduce_their_hashes(filled):
    import hashlib
    for key in ("A", "B"):
        plane = filled_plane(filled, key)
        assert hashlib.sha256(plane.tobytes()).hexdigest() == str(filled[key + "_sha256"]), key
    b = filled_plane(filled, "B")
    v = b[b != -9999]
    assert v.min() < 0 and v.max() > 4000 and (b == -9999).any()      # over the whole clamp and past both ends, with NODATA


def test_filled_windows_are_what_they_claim(filled):
    """The pinned windows: an 8 x 8 interior block (every phase of the 64- and 32-grid maps), one window over each plane edge, the
    corners, an interior NODATA pixel -- and most of them unsaturated, so a probability carries its logit."""
    for key in ("A", "B"):
        H, W = int(filled[key + "_H"]), int(filled[key + "_W"])
        idx, kind = filled[key + "_idx"], filled[key + "_kind"]
        r, c = idx // W, idx % W
        blk = kind == "block"
        assert blk.sum() == 64 and r[blk].min() >= 128 and r[blk].max() <= H - 129 and c[blk].min() >= 128 and c[blk].max() <= W - 129
        assert len({(a & 7, b & 7) for a, b in zip(r[blk], c[blk])}) == 64
        over = np.stack([r < 128, r > H - 129, c < 128, c > W - 129], 1)
        assert all(over[kind == "edge_" + e].sum() == 1 for e in ("top", "bottom", "left", "right"))
        assert sorted(zip(r[kind == "corner"], c[kind == "corner"])) == [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
        p = filled[key + "_prob"]
        assert (p == -9999).sum() >= 1 and (p == -9999).sum() == (filled_plane(filled, key).reshape(-1)[idx] == -9999).sum()
        v = p[p != -9999]
        assert np.mean((v > 1e-3) & (v < 1 - 1e-3)) >= 0.8, key
    assert int(filled["A_block"][0]) > 512 and int(filled["A_H"]) > 512 + 8    # plane A's block is served by rebuilt phase maps


def test_oracle_matches_reference_on_filled_windows(filled, sd):
    for key in ("A", "B"):
        plane, idx = filled_plane(filled, key), filled[key + "_idx"]
        sums = {}
        logits = _oracle_windows(plane, idx, sd, sums)
        np.testing.assert_allclose(logits.numpy(), filled[key + "_logits"], rtol=2e-5, atol=2e-5)
        p, want = _prob(logits, plane, idx), filled[key + "_prob"]
        assert np.array_equal(p == -9999, want == -9999)
        np.testing.assert_allclose(p, want, rtol=1e-4, atol=1e-6)
        for n, a in sums.items():
            np.testing.assert_allclose((a / len(idx)).float().numpy(), filled[key + "_act_mean_" + n], rtol=1e-4, atol=1e-5,
                                       err_msg=key + " " + n)


def test_filled_golden_sees_fp16_operand_errors(filled, sd, monkeypatch):
    """The error class the split route exists to avoid: convolutions on fp16-rounded operands (no lo half).  On windows full of
    data the oracle so changed must miss the golden by >= 5x the 1e-4 bar, measured as the GPU tests measure (relative on p and
    on 1 - p) -- else the golden could not tell the split route from a plain fp16 one."""
    import torch.nn.functional as F
    conv = F.conv2d
    monkeypatch.setattr(F, "conv2d", lambda x, w, *a, **k: conv(x.half().float(), w.half().float(), *a, **k))
    worst = 0.0
    for key in ("A", "B"):
        plane, idx = filled_plane(filled, key), filled[key + "_idx"]
        p, want = _prob(_oracle_windows(plane, idx, sd), plane, idx).astype(np.float64), filled[key + "_prob"].astype(np.float64)
        v = want != -9999
        worst = max(worst, float((np.abs(p[v] - want[v]) / np.minimum(want[v], 1 - want[v])).max()))
    print("fp16-operand oracle against the filled golden: max relative error %.2e" % worst)
    assert worst >= 5e-4, worst


def test_fcn_oracle_matches_reference_on_a_filled_plane(golden_dir, sd):
    """The FCN golden of a 160 x 192 plane full of data (larger than one window; gen_golden_fcn.py --filled)."""
    g = np.load(os.path.join(golden_dir, "cnn_fcn_filled_golden.npz"))
    plane = cnn_weights.synthetic_filled_plane(int(g["H"]), int(g["W"]), seed=int(g["seed_plane"]))
    assert np.array_equal(plane, g["plane"])
    torch.set_num_threads(8)
    sal, stack = O.fcn_predict_plane(plane, sd, float(g["mean"]), float(g["std"]), scale=int(g["scale"]))
    np.testing.assert_allclose(stack, g["predstack"], rtol=1e-5, atol=1e-9)
    assert np.array_equal(sal == -9999, g["saliency"] == -9999)
    np.testing.assert_allclose(sal, g["saliency"], rtol=1e-5, atol=1e-9)

"""GPU parity of the CNN tile scorer (HIP kernels through the C ABI) against goldens made by the reference's own
classes (googlenet1.GoogLeNet, cnn_pred_pipeline.ClampCH4 / FlightlineConvolve) and against the torch-CPU oracle.

float32 network: the bar is 1e-4 relative on the saliency (softmax probability) with NODATA placement exact;
preprocessing (clamp / normalize / pad / window) is bit-exact."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cnn_oracle as O  # noqa: E402
from srcfinder_amd import cnn  # noqa: E402
from srcfinder_amd.cnn_weights import synthetic_plane, synthetic_state_dict  # noqa: E402

MEAN, STD = cnn.MODEL_NORM["COVID_QC"]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cnn_googlenet_golden.npz"))


@pytest.fixture(scope="module")
def net():
    import torch
    assert torch.cuda.is_available()
    return cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024))


def test_clampch4_contract():
    c = cnn.ClampCH4(vmin=0, vmax=4000)
    assert repr(c) == "ClampCH4(vmin=0, vmax=4000)"
    with pytest.raises(AssertionError):
        cnn.ClampCH4(vmin=0.5, vmax=4000)
    with pytest.raises(AssertionError):
        cnn.ClampCH4(vmin=10, vmax=5)


def test_flightline_convolve_bit_exact(gold):
    tf = cnn.Compose([cnn.ClampCH4(vmin=0, vmax=4000), cnn.Normalize([MEAN], [STD])])
    ds = cnn.FlightlineConvolve(gold["plane40"], transform=tf)
    assert len(ds) == 40 * 30 and ds.dim == 256 and tuple(ds.inshape) == (1, 40, 30)
    assert np.array_equal(ds.x.cpu().numpy(), gold["padded40"])
    for k, i in enumerate(gold["tiles_idx"]):
        assert np.array_equal(ds[int(i)].cpu().numpy(), gold["tiles"][k])


def test_activations_and_probabilities(gold, net):
    import torch
    ds = cnn.FlightlineConvolve(gold["plane40"], "COVID_QC")
    idx = [int(i) for i in gold["logits_idx"]]
    probs, means = [], {}
    for j, i in enumerate(idx):
        taps = {}
        out = net.forward_tiles(ds.x, 30, i, 1, taps=taps)
        probs.append(float(out[i].item()))
        for n, a in taps.items():                      # NHWC [1,H,W,C]
            means.setdefault(n, []).append(a.mean(dim=(0, 1, 2)).cpu().numpy())
        if j == 0:
            np.testing.assert_allclose(taps["conv1"][0, :, :, 0].cpu().numpy(), gold["conv1_tile0_ch0"], rtol=1e-5, atol=1e-6)
            got3a = taps["inception3a"][0].permute(2, 0, 1)[:, ::4, ::4].cpu().numpy()
            np.testing.assert_allclose(got3a, gold["inception3a_tile0"], rtol=1e-4, atol=5e-5)   # fp32 noise next to ReLU zeros
    for n, lst in means.items():
        np.testing.assert_allclose(np.mean(lst, axis=0), gold["act_mean_" + n], rtol=1e-4, atol=1e-5)
    want = torch.softmax(torch.as_tensor(gold["logits"]), dim=1)[:, 1].numpy()
    np.testing.assert_allclose(np.array(probs), want, rtol=1e-4, atol=1e-7)


def test_predict_flightline_matches_reference_loop(gold, net):
    sal = cnn.predict_flightline(gold["plane24"], "COVID_QC", net=net, batch=64, to_numpy=True)
    want = gold["saliency24"]
    assert sal.shape == want.shape and sal.dtype == np.float32
    assert np.array_equal(sal == -9999, want == -9999)
    v = want != -9999
    np.testing.assert_allclose(sal[v], want[v], rtol=1e-4, atol=1e-7)


def test_batch_split_and_row_shard_invariance(gold, net):
    """Tiles are independent: batch size and row sharding must not change any value."""
    import torch
    plane = synthetic_plane(9, 13, seed=3)
    a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=117)
    b = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=5)
    assert torch.equal(a, b)
    top = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=32, rows=(0, 4))
    bot = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=32, rows=(4, 9))
    assert torch.equal(torch.cat([top[:4], bot[4:]]), a)
    o = O.predict_plane(plane, synthetic_state_dict(seed=2024), MEAN, STD, indices=[0, 50, 116])
    np.testing.assert_allclose(a.reshape(-1)[[0, 50, 116]].cpu().numpy(), o, rtol=1e-4, atol=1e-7)


def test_fused_conv1_pool_matches_the_two_kernels(net):
    """The production tile scorer evaluates conv1 + maxpool1 in one kernel (implicit GEMM on the matrix cores, the conv1
    activation stays in LDS); the two-kernel form (VALU conv1, then the pool) is what the activation taps use.  Same
    values up to the order of the 49-term fp32 sums -- on interior tiles and on tiles that hang over every image border."""
    import ctypes as C
    import torch
    from srcfinder_amd import _ffi
    L = _ffi.lib()
    plane = synthetic_plane(7, 9, seed=11)
    ds = cnn.FlightlineConvolve(plane, (MEAN, STD), device=net.device)
    Hp, Wp = ds.x.shape[-2], ds.x.shape[-1]
    w, b = net.w["conv1"]
    n = 7 * 9
    a1 = torch.empty((n, 128, 128, 64), dtype=torch.float32, device=net.device)
    p_ref = torch.empty((n, 64, 64, 64), dtype=torch.float32, device=net.device)
    p_fused = torch.full((n, 64, 64, 64), float("nan"), dtype=torch.float32, device=net.device)
    st = _ffi.stream_ptr()
    _ffi.check(L.sf_cnn_conv1(_ffi.ptr(ds.x), Hp, Wp, 9, C.c_longlong(0), n, _ffi.ptr(w), _ffi.ptr(b), _ffi.ptr(a1), st), "conv1")
    _ffi.check(L.sf_cnn_maxpool(_ffi.ptr(a1), n, 128, 128, 64, 3, 2, 0, _ffi.ptr(p_ref), 64, 64, st), "maxpool")
    _ffi.check(L.sf_cnn_conv1_pool(_ffi.ptr(ds.x), Hp, Wp, 9, C.c_longlong(0), n, _ffi.ptr(w), _ffi.ptr(b), _ffi.ptr(p_fused), st),
               "conv1_pool")
    torch.cuda.synchronize()
    assert torch.isfinite(p_fused).all()
    scale = float(p_ref.abs().max())
    assert float((p_fused - p_ref).abs().max()) <= 2e-6 * scale
    assert float(p_ref.max()) > 0          # ReLU outputs: something is active


def test_c_driver_equals_the_python_sequenced_graph_at_route_sized_workspaces(gold):
    """sf_cnn_score_rows (the whole graph for a row range in one C call, weights as one packed blob) against the same
    kernels sequenced from Python (forward_tiles): bit-identical saliency maps, row ranges and ragged last batches."""
    import torch
    from srcfinder_amd import _ffi
    net = cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024))
    plane = synthetic_plane(11, 7, seed=9)
    plane[2, 3] = -9999.0
    a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=13, route="split_unshared")     # C driver
    net.c_driver = False
    b = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=13, route="split_unshared")
    net.c_driver = True
    assert torch.equal(a, b) and float(a[2, 3]) == -9999.0
    c = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=64, rows=(3, 8), route="split_unshared")
    assert torch.equal(c[3:8], a[3:8]) and float(c[:3].abs().sum()) == 0.0
    # the default route shares the trunk up to conv3 between the windows (C driver only): the same map inside float32 rounding,
    # and row ranges / batch sizes still do not change a bit
    d = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=13)
    assert torch.equal(d, a)                             # (bit-identical: the shared form sums in the per-window kernels' order)
    e = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=64, rows=(3, 8))
    assert torch.equal(e[3:8], d[3:8]) and float(e[:3].abs().sum()) == 0.0
    L = _ffi.lib()
    assert net.packed_blob().numel() == L.sf_cnn_blob_floats() and L.sf_cnn_score_workspace_bytes(13, 0, 0, 0) > 0
    assert L.sf_cnn_score_workspace_bytes(13, 11, 7, 0) > L.sf_cnn_score_workspace_bytes(13, 0, 0, 0)
    assert L.sf_cnn_score_workspace_bytes(13, 11, 7, 3) == L.sf_cnn_score_workspace_bytes(13, 0, 0, 3)    # (no sharing buffers)
    assert L.sf_cnn_score_rows(None, None, 4, 4, 0, 4, None, None, 8, 0, None, None, None, 0, None) == -1   # argument errors, no launch


def test_kernel_forms_of_the_tile_scorer_agree_bit_for_bit(gold):
    """The production kernels against their other forms (sf_debug_set keys 16-18): the 8 x 8 conv1+pool kernel with the
    conv tile in LDS, the pointer-form tile fetch of the convolutions, the branch-4 pool as its own launch (strip kernel /
    general kernel: production takes it from the tile staged in LDS, k_poolconv) or inside the 1x1 convolution's fetch.
    Max and the per-output summation order are the same in every form: equal saliency maps."""
    import torch
    from srcfinder_amd import _ffi
    net = cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024))
    plane = synthetic_plane(9, 6, seed=12)
    plane[4, 1] = -9999.0
    ref = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=27)
    L = _ffi.lib()
    for key, val in ((16, 1), (18, 1), (18, 2), (18, 3)):
        L.sf_debug_set(key, val)
        try:
            got = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=27)
        finally:
            L.sf_debug_set(key, 0)
        assert torch.equal(got, ref), (key, val)
    # the pointer-form tile fetch belongs to the direct fp32 kernel (17 = 2; the default convolves by operand splitting)
    both = []
    for val in (2, 1):
        L.sf_debug_set(17, val)
        try:
            both.append(cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=27))
        finally:
            L.sf_debug_set(17, 0)
    assert torch.equal(both[0], both[1])


def test_split_operand_and_winograd_convolutions_against_the_direct_kernel(gold):
    """Three routes for the convolutions of the trunk, all in the float32 tolerance class: operand splitting on the fp16 matrix cores
    (csrc/cnn_split.hip: fp16 hi + lo halves = 22 mantissa bits, three MFMAs, fp32 accumulate; the default), Winograd F(2 x 2, 3 x 3)
    on the fp32 matrix cores for the 3 x 3 layers (csrc/cnn_wino.hip; sf_debug_set(17, 4)), and the direct fp32 implicit GEMM for
    everything (17 = 2).  The saliency maps agree inside the parity bar (1e-4; every route holds the reference goldens at that bar
    in test_activations_and_probabilities), NODATA placement exact, through the Python-sequenced graph and through the C driver."""
    import torch
    from srcfinder_amd import _ffi
    net = cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024))
    assert len(net.wino) == 19                       # conv3 + the 9 branch2 + the 9 branch3 3 x 3 layers
    assert len(net.split) == 38                      # conv2, conv3, 9 x (head3, branch2.1, branch3.1, branch4.1)
    plane = synthetic_plane(10, 7, seed=21)
    plane[3, 2] = -9999.0
    L = _ffi.lib()
    runs = {}
    for c_driver in (True, False):
        net.c_driver = c_driver
        for knob, name in ((0, "split_unshared"), (4, "winograd"), (2, "direct")):
            runs[(c_driver, knob)] = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=32, route=name)
    net.c_driver = True
    # the tools' way in -- the calling thread's tuning knob 17 -- selects the same routes when no route is passed
    L.sf_debug_set(17, 4)
    try:
        assert torch.equal(cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=32), runs[(True, 4)])
    finally:
        L.sf_debug_set(17, 0)
    for knob in (0, 4, 2):
        assert torch.equal(runs[(True, knob)], runs[(False, knob)]), knob
    b = runs[(True, 2)]
    for knob in (0, 4):
        a = runs[(True, knob)]
        assert float(a[3, 2]) == -9999.0 and torch.equal(a == -9999.0, b == -9999.0)
        v = a != -9999.0
        assert not torch.equal(a, b)                     # a different algorithm ...
        rel = float(((a[v] - b[v]).abs() / b[v].abs().clamp_min(1e-7)).max())
        print("route %d vs direct: max relative difference of the saliency %.2e" % (knob, rel))
        assert rel < 1e-4                                # ... the same numbers inside the parity bar (float32 rounding through 57 layers)


def test_shared_trunk_against_every_window_on_its_own(net):
    """Round 6 (csrc/cnn_share.hip; cnn_pred_pipeline.py:53-58, googlenet1.py:110-120): conv1 .. conv3 of a window equal the same
    stack run fully convolutionally over the whole padded plane at the window's phase, except on the ring that sees the window's
    zero padding.  (i) Kernel level, through the C ABI: maxpool2's output assembled from phase maps + ring tensors against the
    per-window kernels (conv1+pool -> conv2 -> conv3 -> maxpool2) for windows of all 16 phases in the middle of a plane larger
    than a window and for windows hanging over the plane's corners.
    (ii) Saliency of whole rows through sf_cnn_score_rows: routes "split" (shared through inception3b) and "split_conv3" against
    "split_unshared" -- bit-identical, with every batch on the shared trunk."""
    import ctypes as C
    import torch
    from srcfinder_amd import _ffi
    L = _ffi.lib()
    P, st = _ffi.ptr, _ffi.stream_ptr
    dev = net.device
    H, W = 300, 290
    plane = synthetic_plane(H, W, seed=17)
    ds = cnn.FlightlineConvolve(plane, (MEAN, STD), device=dev)
    Hp, Wp = H + 255, W + 255
    f32 = dict(dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    w1, b1 = net.w["conv1"]
    h2, l2, s2 = net.split["conv2"]
    h3, l3, s3 = net.split["conv3"]
    b2, b3 = net.w["conv2"][1], net.w["conv3"][1]
    for r0 in (148, 0, 296):                            # interior rows; rows whose windows hang over the top / bottom of the plane
        Rb = r0 >> 2
        rows = 4
        Hq, Wq = ((rows + 3) >> 2) + 1 + 64, ((W - 1) >> 2) + 64
        Hc, Wc = 4 * Hq, 4 * Wq
        q2 = torch.zeros(16 * Hq * Wq * 64 + 64 * 252 * 64 + 4096, **f32)          # maps, then the border tensor of <= 63 windows
        q3all = torch.empty(16 * Hq * Wq * 192 + 20 * 496 * 192, **f32)            # conv3's maps with the ring tensor right behind them
        q3 = q3all[:16 * Hq * Wq * 192].view(16, Hq, Wq, 192)
        canvas = torch.empty((Hc, Wc), **f32)
        c1 = torch.empty((Hc // 2, Wc // 2, 64), **f32)
        p1 = torch.empty((Hq, Wq, 64), **f32)
        for ph in range(16):
            _ffi.check(L.sf_cnn_phase_canvas(P(ds.x), Hp, Wp, 4 * Rb + (ph >> 2), ph & 3, Hc, Wc, P(canvas), st()), "canvas")
            _ffi.check(L.sf_cnn_conv1_image(P(canvas), 1, Hc, Wc, P(w1), P(b1), P(c1), 0, st()), "conv1_image")
            _ffi.check(L.sf_cnn_maxpool(P(c1), 1, Hc // 2, Wc // 2, 64, 3, 2, 0, P(p1), Hq, Wq, st()), "pool1")
            m2 = q2[ph * Hq * Wq * 64:(ph + 1) * Hq * Wq * 64]
            _ffi.check(L.sf_cnn_conv_split(P(p1), 0, 1, Hq, Wq, 64, 64, P(h2), P(l2), P(s2), P(b2), 64, 1, C.c_float(1.0), P(m2), 1,
                                           C.c_float(1.0), 64, 0, P(flag), st()), "conv2 map")
            _ffi.check(L.sf_cnn_conv_split(P(m2), 1, 1, Hq, Wq, 64, 64, P(h3), P(l3), P(s3), P(b3), 192, 3, C.c_float(1.0), P(q3[ph]), 0,
                                           C.c_float(1.0), 192, 0, P(flag), st()), "conv3 map")
        for c0 in (0, 117, W - 20):                     # 20 consecutive windows: every column phase, the plane's left / right edges
            n = 20
            for rr in range(r0, min(H, r0 + rows)):
                tile0 = rr * W + c0
                # every window on its own
                a1 = torch.empty((n, 64, 64, 64), **f32)
                a2 = torch.empty((n, 64, 64, 64), **f32)
                a3 = torch.empty((n, 64, 64, 192), **f32)
                want = torch.empty((n, 32, 32, 192), **f32)
                _ffi.check(L.sf_cnn_conv1_pool(P(ds.x), Hp, Wp, W, C.c_longlong(tile0), n, P(w1), P(b1), P(a1), st()), "conv1_pool")
                _ffi.check(L.sf_cnn_conv_split(P(a1), 0, n, 64, 64, 64, 64, P(h2), P(l2), P(s2), P(b2), 64, 1, C.c_float(1.0), P(a2), 1,
                                               C.c_float(1.0), 64, 0, P(flag), st()), "conv2")
                _ffi.check(L.sf_cnn_conv_split(P(a2), 1, n, 64, 64, 64, 64, P(h3), P(l3), P(s3), P(b3), 192, 3, C.c_float(1.0), P(a3), 0,
                                               C.c_float(1.0), 192, 0, P(flag), st()), "conv3")
                _ffi.check(L.sf_cnn_maxpool(P(a3), n, 64, 64, 192, 3, 2, 0, P(want), 32, 32, st()), "pool2")
                # shared
                ring_off = 16 * Hq * Wq * 64
                p1r = torch.empty((n, 252, 64), **f32)
                c2r = q2[ring_off:ring_off + n * 252 * 64]
                c3r = q3all[16 * Hq * Wq * 192:].view(n, 496, 192)
                got = torch.empty((n, 32, 32, 192), **f32)
                _ffi.check(L.sf_cnn_ring_pool1(P(ds.x), Hp, Wp, W, C.c_longlong(tile0), n, P(w1), P(b1), P(p1r), st()), "ring_pool1")
                _ffi.check(L.sf_cnn_conv_split(P(p1r), 0, 1, 1, n * 252, 64, 64, P(h2), P(l2), P(s2), P(b2), 64, 1, C.c_float(1.0), P(c2r),
                                               1, C.c_float(1.0), 64, 0, P(flag), st()), "conv2 ring")
                _ffi.check(L.sf_cnn_conv_ring(P(q2), 1, C.c_longlong(tile0), n, W, Rb, Hq, Wq, C.c_size_t(ring_off), 2, 64, 1, 1, 2, 2, 64,
                                              P(h3), P(l3), P(s3), P(b3), 192, 0, 0, 3, C.c_float(1.0), P(c3r), 192, 0, None, 0, 0, None, 0, 0,
                                              0, C.c_float(1.0), C.c_float(1.0), P(flag), st()), "conv3 ring")
                _ffi.check(L.sf_cnn_pool_gather(P(q3), C.c_longlong(tile0), n, W, Rb, Hq, Wq, C.c_size_t(q3.numel()), 2, 64, 2, 2, 192, 2,
                                                32, -1, 0, P(got), st()), "pool2 from the maps + ring")
                torch.cuda.synchronize()
                # the border of maxpool1 first (exactly the per-window kernel's values up to the order of conv1's sums)
                border = torch.cat([a1[:, 0, :, :], a1[:, 63, :, :], a1[:, 1:63][:, :, [0, 63], :].reshape(n, 124, 64)], 1)
                scale1 = float(border.abs().max())
                assert float((p1r - border).abs().max()) <= 3e-6 * scale1, (r0, c0, rr)
                scale = float(want.abs().max())
                assert scale > 0 and float((got - want).abs().max()) <= 2e-5 * scale, (r0, c0, rr, float((got - want).abs().max()) / scale)
    assert int(flag.item()) == 0
    # (ii) whole rows through the C driver: shared through inception3b ("split", the default), through conv3 ("split_conv3"), not at all
    for rows in ((144, 153), (0, 2), (298, 300)):
        b = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=96, rows=rows, route="split_unshared")
        for name in ("split", "split_conv3"):
            info = {}
            a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=96, rows=rows, route=name, info=info)
            assert info["shared_batches"] == info["batches"] >= -(-(rows[1] - rows[0]) * W // 96) and info["rescued_batches"] == 0   # every batch on the shared trunk
            sa, sb = a[rows[0]:rows[1]], b[rows[0]:rows[1]]
            v = sb != -9999.0
            assert torch.equal(sa == -9999.0, ~v)
            # every kernel of the shared form sums in the order of its per-window counterpart (conv1's ring kernel included): the maps
            # are the same BITS as every window evaluated on its own
            assert torch.equal(sa, sb), (rows, name, float(((sa[v] - sb[v]).abs() / sb[v].abs().clamp_min(1e-7)).max()))


def test_shared_trunk_rebuilds_its_maps_across_strips_at_flightline_width(net):
    """One call over more image rows than a set of phase maps serves (512 at flightline width): the driver rebuilds the maps when a
    batch leaves the strip -- 540 rows x 598 columns = 323 k windows, batches that straddle image rows and the strip boundary.  The map
    equals the unshared route's bit for bit, and every batch ran on the shared trunk."""
    import torch
    H, W, r0, r1, batch = 1100, 598, 500, 1040, 1000
    plane = synthetic_plane(H, W, seed=23)
    info = {}
    a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, rows=(r0, r1), route="split", info=info)
    b = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, rows=(r0, r1), route="split_unshared")
    assert info["shared_batches"] == info["batches"] >= -(-(r1 - r0) * W // batch) and info["rescued_batches"] == 0
    assert torch.equal(a, b)
    assert float(a[:r0].abs().sum()) == 0.0 and float(a[r1:].abs().sum()) == 0.0
    # anchored to the reference arithmetic (not only to the other route): interior windows on both sides of the map rebuilds
    idx = [505 * W + 130, 640 * W + 301, 777 * W + 468, 850 * W + 200, 903 * W + 377, 971 * W + 129]
    want = O.predict_plane(plane, synthetic_state_dict(seed=2024), MEAN, STD, indices=idx)
    _p_error(a.reshape(-1)[idx].cpu().numpy(), want, "flightline-width strip")
    # the call above scored two halves of the rows concurrently on two streams (cnn.LANES); one stream gives the same bits
    i1 = {}
    c = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, rows=(r0, r1), route="split", info=i1, lanes=1)
    assert info["batches"] == i1["batches"] + 1 and i1["batches"] == -(-(r1 - r0) * W // batch)      # (two short last batches instead of one)
    assert torch.equal(a, c)


def test_band_sharing_equals_the_whole_rings_and_the_unshared_route(net):
    """Round 6, band sharing: the ring rows that see only a window's top / bottom padding come from strip maps built once per 16 image
    rows, per window only the side columns are computed (csrc/cnn_ring.h, cnn_driver.hip::build_strips).  Same bits as the rings
    computed whole (sf_debug_set(16, 3)) and as every window on its own -- across a strip-map boundary (rows 12 .. 20), with batches
    that straddle image rows, and at a width where one batch spans more image rows than a strip group (21 columns, batch 700)."""
    import torch
    from srcfinder_amd import _ffi
    for (H, W, rows, batch) in ((40, 70, (12, 21), 96), (60, 21, (3, 58), 700)):
        plane = synthetic_plane(H, W, seed=31 + W)
        info = {}
        a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, rows=rows, route="split", info=info)
        assert info["shared_batches"] == info["batches"] >= -(-(rows[1] - rows[0]) * W // batch) and info["rescued_batches"] == 0
        try:
            assert _ffi.lib().sf_debug_set(16, 3) == 0
            whole = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, rows=rows, route="split")
        finally:
            _ffi.lib().sf_debug_set(16, 0)
        own = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=batch, rows=rows, route="split_unshared")
        assert torch.equal(a, whole) and torch.equal(a, own), (H, W)


def _scaled_family(sd, k):
    """The weight family with every activation of the trunk multiplied by s = 2^k and the same logits: conv1's folded weight and
    every folded bias times s (ReLU and max pooling are positively homogeneous), fc.weight divided by s.  In state_dict terms:
    conv1.bn.{weight, bias} *= s; every other bn.{bias, running_mean} *= s.  Powers of two: the float32 reference computes the
    same mantissas, so the reference goldens / the torch-CPU oracle of the unscaled family are the oracle of the scaled one."""
    s = float(2.0 ** k)
    out = {}
    for name, v in sd.items():
        v = np.array(v, copy=True)
        if name in ("conv1.bn.weight", "conv1.bn.bias"):
            v = v * s
        elif (name.endswith(".bn.bias") or name.endswith(".bn.running_mean")) and not name.startswith("conv1."):
            v = v * s
        elif name == "fc.weight":
            v = v / s
        out[name] = v.astype(np.float32) if v.dtype.kind == "f" else v
    return out


def test_split_operand_overflow_is_rescued_inside_the_call():
    """An activation at or beyond 65504 has no float16 half: the split-operand launch raises ITS batch's overflow slot and the call
    scores that batch again on the fp32 matrix cores -- through the C driver (sf_cnn_score_rows) and through the Python-sequenced
    graph (score_tiles).  Weights blown up by 1e5 with the scales pinned to 1 make every window overflow: the map equals the fp32
    route's bit for bit, with a warning, and `info` counts the batches.  With the calibrated scales (the default) the same network
    needs no rescue at all: the overflow was a matter of scale."""
    import warnings
    import torch
    from srcfinder_amd import _ffi
    sd = synthetic_state_dict(seed=7)
    sd = {k: (v * 1e5 if k == "conv1.conv.weight" else v) for k, v in sd.items()}
    net = cnn.GoogLeNetHIP(sd)
    plane = synthetic_plane(6, 5, seed=2)
    ones = [1.0] * _ffi.lib().sf_cnn_num_scales()
    want = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=16, route="winograd")
    for c_driver in (True, False):
        net.c_driver = c_driver
        info = {}
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            got = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=16, scales=ones, info=info)
        assert any("float16 range" in str(w.message) for w in wlist)
        assert info["rescued_batches"] == 2 and info["route"] == 0          # 30 windows in batches of 16
        assert torch.equal(got, want)
    net.c_driver = True
    info = {}
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        cal = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=16, info=info)
    assert info["rescued_batches"] == 0 and not wlist and min(info["scales"]) < 1.0
    v = want != -9999.0
    assert float(((cal[v] - want[v]).abs() / want[v].abs().clamp_min(1e-7)).max()) < 1e-4
    # a direct forward_tiles call without a slot checks its own (one synchronisation) and rescues itself
    net.ascale = ones
    ds = cnn.FlightlineConvolve(plane, (MEAN, STD), device=net.device)
    out = torch.zeros(30, dtype=torch.float32, device=net.device)
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        net.forward_tiles(ds.x, 5, 0, 30, plane=ds.plane, out=out)
    assert any("float16 range" in str(w.message) for w in wlist) and torch.equal(out.view(6, 5), want)


def test_overflow_slots_are_per_call_threads_and_streams_do_not_interfere():
    """VERDICT r5 weak 1 / ADVICE r5: route and overflow flag are per call.  (i) gpus=[0, 0, 0] -- three host threads, three
    networks, one device -- on a tall plane whose ONLY bright pixel sits in the last block of rows, weights and pinned scales such
    that exactly the windows that see that pixel overflow: the third thread rescues its batches, the other two none, and the map
    equals the single-threaded call's bit for bit (batch boundaries aligned with the blocks).  (ii) two streams on one device, one
    scoring overflowing windows and one clean ones at the same time, each with its own slot: only the first slot is raised."""
    import torch
    from srcfinder_amd import _ffi
    sd = synthetic_state_dict(seed=7)
    sd = {k: (v * 1e4 if k == "conv1.conv.weight" else v) for k, v in sd.items()}
    ones = [1.0] * _ffi.lib().sf_cnn_num_scales()
    H, W, B = 390, 2, 20                                  # 3 blocks of 130 rows = 260 windows = 13 batches each
    plane = np.full((H, W), np.float32(MEAN), np.float32)   # normalises to 0: a window without the bright pixel sees only biases
    plane[389, 0] = 4000.0                                 # inside the windows of rows >= 262 only
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        i1, i3 = {}, {}
        # (lanes=1: the test's premise is that batch boundaries coincide with the blocks -- a re-scored batch carries the fp32 route's bits)
        single = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=B, scales=ones, info=i1, lanes=1)
        multi = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=B, scales=ones, gpus=[0, 0, 0], info=i3, lanes=1)
        fp32 = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=B, route="winograd")
        clean = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=B, scales=ones, rows=(0, 260), lanes=1)
    assert i3["per_block_rescued"][0] == 0 and i3["per_block_rescued"][1] == 0 and 0 < i3["per_block_rescued"][2] <= 13
    assert i1["rescued_batches"] == i3["rescued_batches"]
    assert torch.equal(single, multi)
    assert torch.equal(multi[380:], fp32[380:])           # the last batch (the bright pixel near the windows' centres): the fp32 route's bits
    assert torch.equal(multi[:260], clean[:260])          # rows no bright pixel reaches: the split route's, untouched
    # (ii) two streams, two slots
    net = cnn.GoogLeNetHIP(sd)
    net2 = cnn.GoogLeNetHIP(sd)
    net.ascale, net2.ascale = ones, ones
    ds = cnn.FlightlineConvolve(plane, (MEAN, STD), device=net.device)
    out = torch.zeros(H * W, dtype=torch.float32, device=net.device)
    slots = net.overflow_slots(2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(sa):
            net.forward_tiles(ds.x, W, 740, 40, plane=ds.plane, out=out, route="split", overflow=slots[0:1])
        with torch.cuda.stream(sb):
            net2.forward_tiles(ds.x, W, 0, 40, plane=ds.plane, out=out, route="split", overflow=slots[1:2])
    torch.cuda.synchronize()
    assert slots.cpu().tolist() == [1, 0]


def test_split_operand_scales_hold_parity_across_the_activation_range(gold):
    """VERDICT r5 missing 5: the reference ships no weights, so the stand-in for "a trained network whose activations live
    elsewhere" is the golden's weight family with every activation scaled by 2^k (see _scaled_family: same logits).  The
    split-operand route with its calibrated per-layer scales holds the reference golden at the golden's 1e-4 for k = -8, +6 and
    -14; with the scales pinned to 1 the low halves of a 2^-14 network are all subnormal and the error is visibly larger."""
    import torch
    from srcfinder_amd import _ffi
    base = synthetic_state_dict(seed=2024)
    want = gold["saliency24"]
    v = want != -9999
    ones = [1.0] * _ffi.lib().sf_cnn_num_scales()
    errs = {}
    for k in (0, -8, 6, -14):
        net = cnn.GoogLeNetHIP(_scaled_family(base, k))
        info = {}
        sal = cnn.predict_flightline(gold["plane24"], "COVID_QC", net=net, batch=64, to_numpy=True, info=info)
        assert np.array_equal(sal == -9999, ~v) and info["rescued_batches"] == 0
        np.testing.assert_allclose(sal[v], want[v], rtol=1e-4, atol=1e-7, err_msg="k = %d" % k)
        errs[k] = float(np.max(np.abs(sal[v] - want[v]) / np.abs(want[v])))
        if k != 0:                                       # the scales follow the family: 2^-k of the unscaled network's
            assert all(abs(a / b - 2.0 ** -k) < 1e-6 for a, b in zip(info["scales"], scales0)), k
        else:
            scales0 = info["scales"]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = cnn.GoogLeNetHIP(_scaled_family(base, -14))
        pinned = cnn.predict_flightline(gold["plane24"], "COVID_QC", net=net, batch=64, to_numpy=True, scales=ones)
    e_pinned = float(np.max(np.abs(pinned[v] - want[v]) / np.abs(want[v])))
    print("max relative saliency error by activation scale 2^k:", errs, "; k = -14 with the scales pinned to 1: %.2e" % e_pinned)
    assert e_pinned > 4 * errs[-14]


def test_winograd_input_of_two_gigabytes_runs_in_image_pieces():
    """The Winograd kernel addresses its input through < 2 GB buffer descriptors; a batch whose activation is larger (conv3 at
    batch 2048: 2.1 GB) is run in pieces of whole images.  The result is the same bits as the same images convolved alone."""
    import torch
    from srcfinder_amd import _ffi
    L = _ffi.lib()
    dev = torch.device("cuda:0")
    N, H, Cin, Cout = 2056, 64, 64, 32
    g = torch.Generator(device="cpu").manual_seed(9)
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * 0.05).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev)
    U = torch.empty(int(L.sf_cnn_wino_weight_floats(Cout, Cin)), dtype=torch.float32, device=dev)
    _ffi.check(L.sf_cnn_wino_weights(_ffi.ptr(w), Cout, Cin, _ffi.ptr(U), _ffi.stream_ptr()), "weights")
    x = torch.empty(N, H, H, Cin, dtype=torch.float32, device=dev)
    assert x.numel() * 4 >= 2 ** 31
    x.normal_(generator=torch.Generator(device=dev).manual_seed(4))
    out = torch.full((N, H, H, Cout), -7.0, dtype=torch.float32, device=dev)
    _ffi.check(L.sf_cnn_conv3x3_wino(_ffi.ptr(x), N, H, H, Cin, Cin, _ffi.ptr(U), _ffi.ptr(bias), Cout, _ffi.ptr(out), Cout, 0,
                                     _ffi.stream_ptr()), "conv3x3_wino")
    for n0 in (0, 1020, 2042, 2052):                 # pieces of 2044 images: the third probe straddles the seam
        xs = x[n0:n0 + 4].contiguous()
        os_ = torch.empty(4, H, H, Cout, dtype=torch.float32, device=dev)
        _ffi.check(L.sf_cnn_conv3x3_wino(_ffi.ptr(xs), 4, H, H, Cin, Cin, _ffi.ptr(U), _ffi.ptr(bias), Cout, _ffi.ptr(os_), Cout, 0,
                                         _ffi.stream_ptr()), "conv3x3_wino")
        assert torch.equal(out[n0:n0 + 4], os_), n0
    assert float(out.min()) >= 0.0                   # every image written (ReLU output; the fill was -7)


def test_gpu_list_scores_row_blocks_from_threads(gold, net):
    """``gpus=[...]`` (the script's ``-g 0 1 ...``, cnn_pred_pipeline.py:113-116): one network and one host thread per
    listed device, contiguous row blocks, assembled once.  On a one-GPU box the list [0, 0, 0] drives the same code with
    three threads on one device: bit-identical to the single call.  A negative index (the reference's CPU run) raises."""
    import torch
    from srcfinder_amd import _ffi
    plane = synthetic_plane(10, 13, seed=5)
    a = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=64)
    sd = synthetic_state_dict(seed=2024)
    b = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=16, gpus=[0, 0, 0])
    assert torch.equal(a, b)
    c = cnn.predict_flightline(plane, (MEAN, STD), weights=sd, batch=64, gpus=[0])
    assert torch.equal(a, c)
    with pytest.raises(_ffi.SrcfinderError):
        cnn.predict_flightline(plane, (MEAN, STD), weights=sd, gpus=[-1])
    with pytest.raises(_ffi.SrcfinderError):
        cnn.predict_flightline(plane, (MEAN, STD), weights=sd, gpus=[0, 97])


def test_cmf_into_cnn_end_to_end(net, library):
    """BASELINE config 4 in miniature: cube -> HIP CMF -> HIP CNN, against oracle CMF -> oracle CNN."""
    import torch
    from oracle import cmf_oracle as CO
    from srcfinder_amd import pipeline
    from srcfinder_amd.synth import make_cube_numpy
    cube = make_cube_numpy(20, 12, seed=31, abscf_full=library[:, 2], nodata_lines=1, nodata_column=5)
    res, sal = pipeline.cmf_then_cnn(torch.as_tensor(cube).cuda(), library, None, net=net, batch=64)
    ref = CO.robust_mf_oracle(cube, library)
    plane = ref["out"][..., 3].astype(np.float32)
    assert np.array_equal(res.out[..., 3].cpu().numpy() == -9999.0, plane == -9999.0)
    idx = [0, 13, 77, 150, 239]
    want = O.predict_plane(plane, synthetic_state_dict(seed=2024), MEAN, STD, indices=idx)
    got = sal.reshape(-1)[idx].cpu().numpy()
    assert np.array_equal(got == -9999, want == -9999)
    v = want != -9999
    np.testing.assert_allclose(got[v], want[v], rtol=2e-4, atol=1e-7)


def test_command_lines_end_to_end(tmp_path, library):
    """The two CLI mirrors on real files: ENVI BIL cube -> robust_mf CLI -> 4-band product (+bgmeta, +csv) ->
    cnn_pred CLI on band 4 -> saliency raster; against the oracles."""
    import torch
    from oracle import cmf_oracle as CO
    from srcfinder_amd import cli_cnn_pred, cli_robust_mf, envi
    from srcfinder_amd.synth import make_cube_numpy
    cube = make_cube_numpy(40, 14, seed=77, abscf_full=library[:, 2], nodata_lines=2, nodata_column=6)
    inp = str(tmp_path / "ang_test_rdn")
    mm = envi.create_image(inp, {"lines": 40, "samples": 14, "bands": 425, "data ignore value": -9999,
                                 "wavelength": ["0"] * 425, "description": "synthetic"}, np.float32, "bil")
    mm[...] = cube
    mm.flush()
    libpath = str(tmp_path / "ang_ch4_unit_3col_425chan.txt")
    np.savetxt(libpath, library, fmt="%.12f")
    outp = str(tmp_path / "ang_test_ch4mf")
    assert cli_robust_mf.main(["-m", inp, libpath, outp]) == 0
    prod, meta = envi.open_memmap(outp)
    assert (meta["lines"], meta["samples"], meta["bands"], meta["data type"], meta["interleave"]) == (40, 14, 4, 5, "bip")
    assert meta["model parameters"] == cmf_params()
    assert "wavelength" not in meta and meta["band names"][3] == "CH4 Absorption (ppm x m)"
    ref = CO.robust_mf_oracle(cube, np.loadtxt(libpath))
    nod = ref["out"][..., 3] == -9999.0
    assert np.array_equal(np.asarray(prod)[..., 3] == -9999.0, nod)
    assert np.array_equal(np.asarray(prod)[..., :3], ref["out"][..., :3])
    np.testing.assert_allclose(np.asarray(prod)[..., 3][~nod], ref["out"][..., 3][~nod], rtol=1e-4, atol=1e-6)
    bg, bmeta = envi.open_memmap(outp + "_bgmeta")
    assert np.array_equal(np.asarray(bg), ref["bgmeta"]) and int(bmeta["num alphas"]) == 201
    rows = open(os.path.splitext(inp)[0] + "_column_stats.csv").read().strip().split("\n")
    assert [r.split(",")[0] for r in rows] == ["", "npix", "avg", "std"]
    assert [float(v) for v in rows[1].split(",")[1:]] == list(ref["colstats"][0])
    # CNN CLI on band 4 of that product
    wpath = str(tmp_path / "COVID_QC.pt")
    sd = synthetic_state_dict(seed=2024)
    torch.save({k: torch.as_tensor(v) for k, v in sd.items()}, wpath)
    assert cli_cnn_pred.main([outp, "-m", "COVID_QC", "-g", "0", "-b", "64", "-o", str(tmp_path), "--band", "4",
                              "--weights", wpath]) == 0
    sal, smeta = envi.open_memmap(str(tmp_path / "ang_test_ch4mf_saliency.img"))
    assert (smeta["lines"], smeta["samples"], smeta["bands"], smeta["data type"]) == (40, 14, 1, 4)
    plane = np.asarray(prod)[..., 3].astype(np.float32)
    idx = [0, 100, 333, 559]
    want = O.predict_plane(plane, sd, MEAN, STD, indices=idx)
    got = np.asarray(sal)[0].reshape(-1)[idx]
    assert np.array_equal(got == -9999, want == -9999)
    v = want != -9999
    np.testing.assert_allclose(got[v], want[v], rtol=2e-4, atol=1e-7)


def cmf_params():
    from srcfinder_amd import cmf
    return cmf.model_parameters(False, (351, 422))


def test_fp16_option_is_close_but_separate(gold):
    """precision="fp16" (float16 operands, fp32 accumulate): NOT the parity path; its own tolerance.
    NODATA placement stays exact; saliency within 5e-3 absolute / 2e-2 relative of the fp32 reference golden."""
    net16 = cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024), precision="fp16")
    sal = cnn.predict_flightline(gold["plane24"], "COVID_QC", net=net16, batch=64, to_numpy=True)
    want = gold["saliency24"]
    assert np.array_equal(sal == -9999, want == -9999)
    v = want != -9999
    np.testing.assert_allclose(sal[v], want[v], rtol=2e-2, atol=5e-3)
    assert np.abs(sal[v] - want[v]).max() > 0          # it really is a different arithmetic


# ---- FCN shift-and-stitch (the reference's approximate fast mode, cnn/fcn_pred_pipeline.py) -------------------------
# --- windows full of data (tests/golden/gen_golden_cnn.py --filled, cnn_googlenet_filled_golden.npz): the flightline case.  The
# goldens above are planes smaller than a window (>= 98 % padding); the tests on large planes compare routes with each other only.
# Bar: relative 1e-4 on p AND on 1 - p (a window at p = 0.99 must not pass at any error), NODATA placement exact.

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


@pytest.mark.parametrize("route", ["split", "split_conv3", "split_unshared", "winograd", "direct"])
def test_every_route_against_the_reference_on_filled_windows(filled, net, route):
    """sf_cnn_score_rows on each route against the filled golden.  Shared routes: ALL rows of a plane in one call, default lanes (2:
    the lane cut falls inside the plane), batch 512 -- plane A (1400 rows) rebuilds its phase maps in both lanes and its pinned block
    straddles a strip-map rebuild; every batch must have run on the shared trunk with none rescued, so no fallback passes unseen.
    Unshared routes: the rows that hold the pinned windows."""
    errs = {}
    for key in ("A", "B"):
        plane, idx = _filled_plane(filled, key), filled[key + "_idx"]
        H, W = plane.shape
        out = np.zeros(H * W, np.float32)
        if route in ("split", "split_conv3"):
            info = {}
            out = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=512, route=route, info=info, to_numpy=True).reshape(-1)
            assert info["shared_batches"] == info["batches"] >= -(-H * W // 512) and info["rescued_batches"] == 0, (key, info)
        else:
            rows = sorted(set((idx // W).tolist()))
            runs, r0 = [], rows[0]
            for a, b in zip(rows, rows[1:] + [None]):
                if b != a + 1:
                    runs.append((r0, a + 1))
                    r0 = b
            for rr in runs:
                got = cnn.predict_flightline(plane, (MEAN, STD), net=net, batch=512, rows=rr, route=route, to_numpy=True)
                out[rr[0] * W:rr[1] * W] = got.reshape(-1)[rr[0] * W:rr[1] * W]
        errs[key] = _p_error(out[idx], filled[key + "_prob"], (route, key))
    print("filled golden, route %s: max |dp| / min(p, 1-p) = A %.2e, B %.2e" % (route, errs["A"], errs["B"]))


def test_python_sequenced_graph_and_its_taps_on_filled_windows(filled, net):
    """forward_tiles (the same kernels sequenced from Python, split operands at the plane's calibrated scales) on every pinned window:
    probabilities at the bar above, and per-layer channel means of the taps against the reference's (1e-4 relative)."""
    import torch
    keep = list(net.ascale)
    try:
        for key in ("A", "B"):
            plane, idx = _filled_plane(filled, key), filled[key + "_idx"]
            W = plane.shape[1]
            ds = cnn.FlightlineConvolve(plane, (MEAN, STD), device=net.device)
            net.calibrate(ds, 64)
            out = torch.zeros(plane.size, dtype=torch.float32, device=net.device)
            runs, a = [], 0                                  # consecutive window indices: one forward_tiles call each
            for b in range(1, len(idx) + 1):
                if b == len(idx) or idx[b] != idx[b - 1] + 1:
                    runs.append((int(idx[a]), b - a))
                    a = b
            sums = {}
            for t0, n in runs:
                taps = {}
                net.forward_tiles(ds.x, W, t0, n, plane=ds.plane, out=out, taps=taps, route="split")
                for name, t in taps.items():                  # NHWC
                    sums[name] = sums.get(name, 0) + t.double().mean(dim=(1, 2)).sum(0)
            err = _p_error(out.cpu().numpy()[idx], filled[key + "_prob"], ("forward_tiles", key))
            layer = {}
            for name, t in sums.items():
                got, want = (t / len(idx)).cpu().numpy(), filled[key + "_act_mean_" + name].astype(np.float64)
                layer[name] = float((np.abs(got - want) / (np.abs(want) + 1e-1)).max())
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5, err_msg="%s %s" % (key, name))
            print("filled golden %s, forward_tiles: p %.2e; per layer max |d| / (|mean| + 0.1): %s" % (
                key, err, " ".join("%s %.1e" % kv for kv in layer.items())))
    finally:
        net.ascale = keep


@pytest.fixture(scope="module")
def fcn_gold(golden_dir):
    return np.load(os.path.join(golden_dir, "cnn_fcn_golden.npz"))


def _logit(p):
    p = np.clip(p.astype(np.float64), 1e-300, 1.0)
    return np.log(p) - np.log1p(-np.minimum(p, 1.0 - 1e-16))


def test_fcn_canvas_is_bit_exact(fcn_gold, net):
    """FlightlineShiftStitch.__getitem__ (:55-65): transform, divisibility pad, shift pad -- one shifted canvas."""
    import torch
    from srcfinder_amd import _ffi
    g = fcn_gold
    H, W, scale = int(g["H"]), int(g["W"]), int(g["scale"])
    Hc, Wc = g["canvas_5_9"].shape
    assert (Hc, Wc) == (H + (scale - H % scale) + scale, W + (scale - W % scale) + scale)
    plane = torch.as_tensor(g["plane"]).cuda()
    out = torch.empty((2, Hc, Wc), dtype=torch.float32, device="cuda")
    _ffi.check(_ffi.lib().sf_cnn_fcn_prepare(_ffi.ptr(plane), H, W, 0.0, 4000.0, float(g["mean"]), float(g["std"]), scale,
                                             5 * scale + 8, 2, Hc, Wc, _ffi.ptr(out), _ffi.stream_ptr()), "prepare")
    assert np.array_equal(out[1].cpu().numpy(), g["canvas_5_9"])


def test_fcn_shift_and_stitch_matches_reference(fcn_gold, net):
    """Whole fast mode against the golden made by the reference's FlightlineShiftStitch / stitch_stack around its
    converted model: NODATA placement exact; probabilities to 2e-6 absolute + 5e-3 relative -- the per-cell logits of
    the un-pooled head reach +-35, so a float32 logit error of 1e-4 relative is up to 4e-3 relative in a saturated
    probability; where the probability is not saturated the logit difference itself is held to 5e-3."""
    g = fcn_gold
    sal = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net, batch=16, to_numpy=True)
    want = g["saliency"]
    assert sal.shape == want.shape and sal.dtype == np.float32
    assert np.array_equal(sal == -9999, want == -9999)
    v = want != -9999
    np.testing.assert_allclose(sal[v], want[v], rtol=5e-3, atol=2e-6)
    mid = v & (want > 1e-3) & (want < 1 - 1e-3)      # a float32 probability closer to 0 or 1 no longer carries its logit
    assert mid.sum() > 100
    assert np.abs(_logit(sal[mid]) - _logit(want[mid])).max() < 5e-3


def test_fcn_batch_and_shift_range_invariance(fcn_gold, net):
    """Batch size does not change a bit; disjoint shift ranges (the multi-GPU split) tile the image exactly."""
    import torch
    g = fcn_gold
    a = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net, batch=16)
    b = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net, batch=5)
    assert torch.equal(a, b)
    lo = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net, batch=16, shifts=(0, 400))
    hi = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net, batch=16, shifts=(400, 1024))
    assert torch.equal(torch.where(lo != 0, lo, hi), a)


def test_fcn_command_line(fcn_gold, tmp_path):
    """cli_fcn_pred on an ENVI raster of the golden plane reproduces the golden saliency raster."""
    import torch
    from srcfinder_amd import cli_fcn_pred, envi
    g = fcn_gold
    H, W = int(g["H"]), int(g["W"])
    inp = str(tmp_path / "ang_fcn_ch4mf")
    mm = envi.create_image(inp, {"lines": H, "samples": W, "bands": 1, "data ignore value": -9999}, np.float32, "bsq")
    mm[0] = g["plane"]
    mm.flush()
    wpath = str(tmp_path / "COVID_QC.pt")
    torch.save({k: torch.as_tensor(v) for k, v in synthetic_state_dict(seed=2024).items()}, wpath)
    assert cli_fcn_pred.main([inp, "-g", "0", "-b", "16", "-o", str(tmp_path), "--weights", wpath]) == 0
    sal, smeta = envi.open_memmap(str(tmp_path / "ang_fcn_ch4mf_saliency.img"))
    assert (smeta["lines"], smeta["samples"], smeta["bands"], smeta["data type"]) == (H, W, 1, 4)
    got, want = np.asarray(sal)[0], g["saliency"]
    assert np.array_equal(got == -9999, want == -9999)
    v = want != -9999
    np.testing.assert_allclose(got[v], want[v], rtol=5e-3, atol=2e-6)


def test_fcn_fp16_option_is_close_but_separate(fcn_gold):
    """precision="fp16" on the FCN path (float16 activations / weights, fp32 accumulation, conv1 on the fp32 VALU): its own
    tolerance -- the un-pooled logits are large, so the comparison is on the logit where float32 can resolve it."""
    g = fcn_gold
    net16 = cnn.GoogLeNetHIP(synthetic_state_dict(seed=2024), precision="fp16")
    sal = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net16, batch=16, to_numpy=True)
    want = g["saliency"]
    assert np.array_equal(sal == -9999, want == -9999)
    v = want != -9999
    mid = v & (want > 1e-3) & (want < 1 - 1e-3)
    d = np.abs(_logit(sal[mid]) - _logit(want[mid]))
    assert d.max() < 0.5 and np.median(d) < 0.05, (d.max(), np.median(d))
    assert np.abs(sal[v] - want[v]).max() > 0                     # it really is a different arithmetic
    assert np.mean((sal[v] > 0.5) == (want[v] > 0.5)) > 0.99      # same side of the decision threshold almost everywhere


def test_fcn_on_a_filled_plane_larger_than_a_window(golden_dir, net):
    """The FCN fast mode on a 160 x 192 plane full of data (gen_golden_fcn.py --filled), on the split and the Winograd routes, at the
    bars of test_fcn_shift_and_stitch_matches_reference."""
    g = np.load(os.path.join(golden_dir, "cnn_fcn_filled_golden.npz"))
    want = g["saliency"]
    v = want != -9999
    mid = v & (want > 1e-3) & (want < 1 - 1e-3)
    assert mid.sum() > 5000
    for route in ("split", "winograd"):
        sal = cnn.fcn_predict_flightline(g["plane"], "COVID_QC", net=net, batch=16, to_numpy=True, route=route)
        assert np.array_equal(sal == -9999, want == -9999), route
        np.testing.assert_allclose(sal[v], want[v], rtol=5e-3, atol=2e-6, err_msg=route)
        d = np.abs(_logit(sal[mid]) - _logit(want[mid]))
        print("filled FCN golden, route %s: max |d logit| %.2e (median %.2e), max |dp| %.2e" % (
            route, d.max(), np.median(d), np.abs(sal[v] - want[v]).max()))
        assert d.max() < 5e-3, (route, d.max())

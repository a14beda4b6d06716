"""No-GPU checks of the CMF-threshold plume detector (srcfinder_util.filtdet :1422-1482, ime :1989-1996).

A numpy / scipy restatement of the reference's rules, written here from the rules alone, reproduces every golden that
the reference itself produced (tests/golden/gen_golden_filtdet.py): it pins the 4-connected ``< minarea`` removal, the
8-connected restore of small strong components and the order-keeping compaction independently of the GPU.  The kernel's
reflect indexing (repeated when the radius reaches past the line) is checked against scipy's here too.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

from srcfinder_amd import _ffi, plumes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sf_image_label4", "sf_plumes_gauss_scratch_bytes", "sf_plumes_gauss_pass", "sf_plumes_threshold",
       "sf_plumes_restore_scratch_bytes", "sf_plumes_restore_small", "sf_plumes_compact_scratch_bytes",
       "sf_plumes_compact", "sf_plumes_stats"]
S4 = ndi.generate_binary_structure(2, 1)
S8 = ndi.generate_binary_structure(2, 2)


# ---- the restatement ----------------------------------------------------------------------------------------------
def prestage(ch4mf, k, skip_kde, use_abs):
    d = np.abs(ch4mf) if use_abs else ch4mf.copy()
    if skip_kde:
        return d
    g = ndi.gaussian_filter(d, sigma=k, truncate=1, mode="reflect")
    return d * ((g - g.min()) / (g.max() - g.min()))


def filtdet_np(ch4mf, nodata, minarea=9, mfmin=500, mfmax=1500, k=50, mfminsmall=1250, skip_kde=False, use_abs=False):
    detkde = np.clip((prestage(ch4mf, k, skip_kde, use_abs) - mfmin) / (mfmax - mfmin), 0.0, 1.0)
    ch4min = ch4mf >= mfmin
    detmask = detkde > 0
    lab4 = ndi.label(detmask, structure=S4)[0]
    kept = detmask & (np.bincount(lab4.ravel())[lab4] >= minarea)          # size < minarea goes
    if mfminsmall >= mfmin:
        small = ndi.label(detmask & ~kept, structure=S8)[0]
        strong = np.unique(small[(ch4mf >= mfminsmall) & (small > 0)])
        kept |= np.isin(small, strong) & (small > 0)
    comp = ndi.label(kept, structure=S8)[0]
    comp[~ch4min] = 0
    surv = np.unique(comp[comp > 0])
    fwd = np.zeros(comp.max() + 1, np.int32)
    fwd[surv] = np.arange(1, len(surv) + 1)
    comp = fwd[comp]
    detkde[~ch4min] = 0
    detkde[nodata] = 0
    comp[nodata] = 0
    return detkde, comp.astype(np.int32)


def table_np(ch4mf, comp, ps):
    rows, vals = [], []
    for i in range(1, int(comp.max()) + 1):
        m = comp == i
        ys, xs = np.nonzero(m)
        v = ch4mf[m]
        j = int(np.argmax(v))
        rows.append([m.sum(), ys.min(), ys.max() + 1, xs.min(), xs.max() + 1, ys[j], xs[j]])
        vals.append([v.sum(), v.max(), v.sum() * plumes.ime_scale(ps)])
    return np.array(rows, np.int64).reshape(-1, 7), np.array(vals).reshape(-1, 3)


def golden_params(g, name):
    p = g["%s_params" % name]
    return dict(minarea=int(p[0]), mfmin=p[1], mfmax=p[2], k=p[3], mfminsmall=p[4], skip_kde=bool(p[5]), use_abs=bool(p[6]))


def load_golden(golden_dir):
    """The goldens with the scene inputs (stored as int16 of twice the half-integer ppm m) as the float64 planes the
    reference ran on."""
    g = dict(np.load(os.path.join(golden_dir, "filtdet_golden.npz")))
    for k in list(g):
        if k.endswith("_ch4mf"):
            g[k] = g[k].astype(np.float64) / 2
    return g


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir)


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srcfinder_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sf_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _ffi.SIGNATURES, name
        assert hasattr(L, name), name
    assert "plumes.hip" in open(os.path.join(ROOT, "srcfinder_amd", "csrc", "Makefile")).read()


def test_entry_points_reject_bad_arguments_without_a_device():
    L = _ffi.lib()
    one = ctypes.c_void_p(16)
    two = ctypes.c_void_p(32)
    w = ctypes.c_void_p(48)
    assert L.sf_plumes_gauss_pass(one, two, 10, 10, 0, w, 193, 0, None, None, None) < 0
    assert b"radius" in L.sf_last_error_string()
    assert L.sf_plumes_gauss_pass(one, one, 10, 10, 0, w, 5, 0, None, None, None) < 0        # in place
    assert L.sf_plumes_gauss_pass(one, two, 10, 10, 2, w, 5, 0, None, None, None) < 0        # axis
    assert L.sf_plumes_gauss_pass(one, two, 10, 10, 0, w, 5, 0, one, one, None) < 0          # min / max on axis 0
    assert L.sf_plumes_threshold(one, one, None, 10, 10, 500.0, 1500.0, 0, one, one, one, None) < 0
    assert L.sf_plumes_restore_small(one, one, None, 1250.0, 10, 10, one, None) < 0
    assert L.sf_plumes_compact(one, None, one, None, None, 10, 10, one, None) < 0
    assert L.sf_plumes_stats(one, one, 10, 10, -1, one, one, None) < 0
    assert L.sf_image_label4(None, 10, 10, one, None, 0, one, one, None) < 0
    assert b"sf_image_label4" in L.sf_last_error_string()
    assert L.sf_plumes_gauss_scratch_bytes(0, 10) == 0
    assert L.sf_plumes_restore_scratch_bytes(598, 20000) > 598 * 20000 * 5
    assert L.sf_plumes_compact_scratch_bytes(598, 20000) >= 299 * 10000 * 4


def test_python_surface_checks_its_arguments():
    z = np.zeros((4, 4))
    with pytest.raises(ValueError, match="mfmax"):
        plumes._check_args(z.shape, 9, 500, 500, 50, False)
    with pytest.raises(ValueError, match="mfmin"):
        plumes._check_args(z.shape, 9, 0, 500, 50, False)
    with pytest.raises(ValueError, match="minarea"):
        plumes._check_args(z.shape, 2.5, 500, 1500, 50, False)
    with pytest.raises(ValueError, match="sigma"):
        plumes._check_args(z.shape, 9, 500, 1500, 0, False)
    with pytest.raises(ValueError, match="radius"):
        plumes._check_args(z.shape, 9, 500, 1500, 500, False)
    with pytest.raises(ValueError, match="2-d"):
        plumes._check_args((4, 4, 4), 9, 500, 1500, 50, False)
    plumes._check_args(z.shape, 9, 500, 1500, 500, True)          # no blur: the sigma is not used
    plumes._check_args(z.shape, 9, 500, 1500, 50, False)


# ---- the rules ----------------------------------------------------------------------------------------------------
def test_ime_scale_is_the_reference_formula(golden):
    for ps in (1.0, 3.1, 5.0, 8.1):
        assert plumes.ime_scale(ps) == (1.0 / 1e6) * ((ps * ps) / 1.0) * (1000.0 / 1.0) * (1.0 / 22.4) * (0.01604 / 1.0)
    assert plumes.ime_scale(float(golden["ps"])) == float(golden["ime_scale_ps"])
    assert plumes.ime(np.array([100.0, 250.5]), 3.1) == 350.5 * plumes.ime_scale(3.1)
    with pytest.raises(ValueError):
        plumes.ime(np.array([1.0, -1.0]), 3.1)
    with pytest.raises(ValueError):
        plumes.ime(np.array([1.0, np.nan]), 3.1)


def test_gaussian_weights_are_scipys():
    for sigma in (1.0, 5.0, 50.0, 7.3):
        w, r = plumes.gaussian_weights(sigma)
        assert r == int(sigma + 0.5) and len(w) == 2 * r + 1
        assert np.array_equal(w, ndi._filters._gaussian_kernel1d(sigma, 0, r))


def _reflect(i, n):                  # the kernel's reflect_idx (csrc/plumes.hip)
    p = 2 * n
    m = i % p
    return m if m < n else p - 1 - m


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 40])
def test_kernel_reflect_indexing_matches_scipy_when_the_radius_exceeds_the_line(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n)
    w, r = plumes.gaussian_weights(12.0)
    want = ndi.correlate1d(x, w, mode="reflect")
    got = np.array([sum(w[j] * x[_reflect(i - r + j, n)] for j in range(2 * r + 1)) for i in range(n)])
    assert np.allclose(got, want, rtol=1e-13, atol=1e-15)


def test_restatement_reproduces_every_reference_golden(golden):
    for name in golden["scenes"]:
        ch4mf, nodata = golden["%s_ch4mf" % name], golden["%s_nodata" % name]
        p = golden_params(golden, name)
        pre = prestage(ch4mf, p["k"], p["skip_kde"], p["use_abs"])
        assert (np.abs(pre - p["mfmin"]) / p["mfmin"]).min() > 1e-9, name
        detkde, comp = filtdet_np(ch4mf, nodata, **p)
        assert np.array_equal(comp, golden["%s_detcomp" % name]), name
        assert np.allclose(detkde, golden["%s_detkde" % name], rtol=1e-12, atol=1e-300), name
        rows, vals = table_np(ch4mf, comp, float(golden["ps"]))
        assert np.array_equal(rows, golden["%s_table_int" % name]), name
        assert np.allclose(vals, golden["%s_table_f" % name], rtol=1e-12, atol=0), name


def test_goldens_pin_the_connectivity_and_size_rules(golden):
    """Counterfactuals: an 8-connected removal, a <= minarea removal or no restore step would each miss a golden."""
    def variant(ch4mf, nodata, p, conn_remove=S4, le=False, restore=True):
        detkde = np.clip((prestage(ch4mf, p["k"], p["skip_kde"], p["use_abs"]) - p["mfmin"]) / (p["mfmax"] - p["mfmin"]), 0, 1)
        m = detkde > 0
        lab = ndi.label(m, structure=conn_remove)[0]
        sizes = np.bincount(lab.ravel())[lab]
        kept = m & ((sizes > p["minarea"]) if le else (sizes >= p["minarea"]))
        if restore and p["mfminsmall"] >= p["mfmin"]:
            small = ndi.label(m & ~kept, structure=S8)[0]
            strong = np.unique(small[(ch4mf >= p["mfminsmall"]) & (small > 0)])
            kept |= np.isin(small, strong) & (small > 0)
        comp = ndi.label(kept, structure=S8)[0]
        comp[(ch4mf < p["mfmin"]) | nodata] = 0
        return comp > 0
    changed = {"conn8": 0, "le": 0, "norestore": 0}
    for name in golden["scenes"]:
        ch4mf, nodata = golden["%s_ch4mf" % name], golden["%s_nodata" % name]
        p = golden_params(golden, name)
        want = golden["%s_detcomp" % name] > 0
        changed["conn8"] += not np.array_equal(variant(ch4mf, nodata, p, conn_remove=S8), want)
        changed["le"] += not np.array_equal(variant(ch4mf, nodata, p, le=True), want)
        changed["norestore"] += not np.array_equal(variant(ch4mf, nodata, p, restore=False), want)
    assert all(v > 0 for v in changed.values()), changed


def test_use_abs_golden_drops_and_renumbers_labels(golden):
    comp = golden["c_detcomp"]
    assert comp.max() > 0 and set(np.unique(comp)) == set(range(comp.max() + 1))
    p = golden_params(golden, "c")
    assert p["use_abs"]
    full = ndi.label(filtdet_np(golden["c_ch4mf"], golden["c_nodata"], **dict(p, mfmin=p["mfmin"]))[1] > 0, structure=S8)[0]
    assert full.max() == comp.max()
    pre = prestage(golden["c_ch4mf"], p["k"], False, True)
    assert ndi.label(pre > p["mfmin"], structure=S8)[0].max() > comp.max()       # labels that the compaction removed

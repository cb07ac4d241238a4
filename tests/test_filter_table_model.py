"""The cfconv filter table on the CPU (tests/filter_table_model.py, a NumPy restatement of the interpolation the table
kernel runs): its float32 interpolant against the float64 filter on the seed-7 weights of all three blocks, the fall-back
decision for extreme weights, exact reproduction at the knots, constant continuation beyond the domain, an offset.

The bar is ``fused.FILTER_TABLE_BAR``: twice the MFMA kernel's own error against float64."""
import numpy as np
import pytest

import filter_table_model as M
from gcnn_keras_amd import synth
from gcnn_keras_amd.fused import FILTER_TABLE_BAR

GAUSS = dict(bins=20, distance=4.0, sigma=0.4)
f32 = np.float32


def _block(i, scale=1.0, seed=7):
    p = synth.schnet_params(seed=seed, random_bias=True)
    pre = "interaction%d/cfconv/" % i
    return ((p[pre + "dense1/kernel"] * f32(scale)).astype(f32), p.get(pre + "dense1/bias"), p[pre + "dense2/kernel"],
            p.get(pre + "dense2/bias"))


def _queries(L, offset=0.0):
    rng = np.random.default_rng(5)
    d = rng.uniform(0.0, 7.5, size=40000).astype(f32)
    end = L["v_end"] + f32(offset)
    return np.concatenate([d, np.array([0.0, 1e-6, end, np.nextafter(end, f32(np.inf)), 10.0, 1e3], f32)])


def _error(block, scale=1.0, offset=0.0, log2_inv_h=5):
    w = _block(block, scale)
    L = M.layout(offset=offset, log2_inv_h=log2_inv_h, **GAUSS)
    table = M.build_table(L, *w, GAUSS["distance"], GAUSS["sigma"])
    d = np.concatenate([_queries(L, offset), M.check_points(L, offset)])
    return M.error_over_scale(table, d, offset, L, *w, GAUSS["distance"], GAUSS["sigma"])


def test_layout_follows_the_domain_rule():
    L = M.layout(offset=0.0, **GAUSS)
    assert float(L["v_lo"]) == 0.0 and L["n_int"] == 212 and L["rows"] == 218 and float(L["inv_h"]) == 32.0
    assert float(L["v_end"]) == 212 / 32.0 >= 4.0 * 19 / 20 + 7 * 0.4
    L = M.layout(offset=0.5, **GAUSS)
    assert float(L["v_lo"]) == -0.5 and L["n_int"] == 228
    L = M.layout(bins=20, distance=2.0, sigma=0.4, offset=5.0)      # the Gaussians' reach, not the offset, ends the domain
    assert abs(float(L["v_lo"]) + 2.8) < 1e-6
    assert M.layout(bins=20, distance=30.0, sigma=0.4, offset=0.0) is None      # would not fit: the route keeps the MFMA kernel


@pytest.mark.parametrize("block", [0, 1, 2])
def test_seed7_blocks_stay_under_the_bar(block):
    err = _error(block)
    print("[filter table] block %d: %.2e of the filter's scale (bar %.2e)" % (block, err, FILTER_TABLE_BAR))
    assert err <= FILTER_TABLE_BAR


def test_extreme_weights_exceed_the_bar_at_the_default_spacing():
    """``W1`` x 20: the table at h = 2^-5 is off by more than the bar - the route then keeps the MFMA kernel (a table at
    h = 2^-6 has 429 rows and does not fit the kernel's LDS)."""
    err = _error(0, scale=20.0)
    print("[filter table] W1 x 20: %.2e at h = 2^-5 (bar %.2e)" % (err, FILTER_TABLE_BAR))
    assert err > FILTER_TABLE_BAR
    assert M.layout(offset=0.0, log2_inv_h=6, **GAUSS) is None


def test_knots_are_reproduced_exactly():
    w = _block(1)
    for offset in (0.0, 0.5):
        L = M.layout(offset=offset, **GAUSS)
        table = M.build_table(L, *w, GAUSS["distance"], GAUSS["sigma"])
        j = np.arange(2, L["n_int"] + 3)                       # the knots inside the domain, both ends included
        d = (M.knots(L)[j] + offset).astype(f32)
        wts, i = M.point(d, offset, L)
        assert np.array_equal(np.sort(wts, axis=1)[:, :5], np.zeros((len(j), 5), f32)) and np.all(wts.max(axis=1) == 1.0)
        assert np.array_equal(M.interpolate(table, d, offset, L), table[j])


def test_constant_beyond_both_ends():
    """A basis whose domain starts at -7 sigma (offset 3 > 7 sigma) and ends at distance 19/20 + 7 sigma."""
    w = _block(2)
    offset, distance, sigma = 3.0, 2.0, 0.4
    L = M.layout(bins=20, distance=distance, sigma=sigma, offset=offset)
    assert abs(float(L["v_lo"]) + 2.8) < 1e-6 and L["n_int"] == 240
    table = M.build_table(L, *w, distance, sigma)
    lo = M.interpolate(table, np.array([0.0, 0.1, offset + float(L["v_lo"]) - 1e-3], f32), offset, L)
    hi = M.interpolate(table, np.array([offset + float(L["v_end"]) + 1e-3, 10.0, 1e3, np.inf], f32), offset, L)
    assert np.array_equal(lo, np.broadcast_to(table[2], lo.shape))
    assert np.array_equal(hi, np.broadcast_to(table[L["n_int"] + 2], hi.shape))
    # ... which is the filter there, to the Gaussians' 2.3e-11
    for v, row in ((-3.0, table[2]), (1e3, table[L["n_int"] + 2])):
        far = M.filter64(np.array([v]), *w, distance, sigma)[0]
        assert np.max(np.abs(far - row)) <= 2.0 ** -23 * np.max(np.abs(far))


def test_offset():
    err = _error(1, offset=0.5)
    print("[filter table] block 1, offset 0.5: %.2e of the filter's scale" % err)
    assert err <= FILTER_TABLE_BAR

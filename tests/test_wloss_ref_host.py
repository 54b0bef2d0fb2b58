"""tests/_wloss_ref.py, the numpy specification of wd_weighted_mse_loss, against torch CPU autograd in float64:

    L = mean_b w_b * sum_i m_bi (p - e)_bi^2 / sum_i m_bi

The specification rounds d = p - e, the scale c_b and two products to fp32 (2^-24 relative each, four of them: 2.4e-7), so L and
every row of dL/dp are held to 1e-6 relative.  Also: the row whose mask is all zero, and the histogram's bin edges.  No GPU."""
import numpy as np
import pytest
import torch

from tests import _wloss_ref as R

T = 1000


def _case(B, n, masked, weighted, seed):
    rs = np.random.RandomState(seed)
    p = rs.standard_normal((B, n)).astype(np.float32)
    e = (0.5 * rs.standard_normal((B, n)) + 0.25).astype(np.float32)
    m = (rs.randint(0, 257, (B, n)) / 256.0).astype(np.float32) if masked else None
    t = rs.randint(0, T, B)
    w = rs.uniform(0.0, 2.0, T).astype(np.float32) if weighted else None
    return p, e, m, t, w


def _autograd(p, e, m, t, w, rows=None):
    """(L, dL/dp) in float64; rows: the samples that count (all by default)."""
    B, n = p.shape
    pt = torch.from_numpy(p).double().requires_grad_(True)
    et = torch.from_numpy(e).double()
    mt = torch.ones(B, n, dtype=torch.float64) if m is None else torch.from_numpy(m).double()
    wt = torch.ones(B, dtype=torch.float64) if w is None else torch.from_numpy(w).double()[torch.from_numpy(t)]
    rows = list(range(B)) if rows is None else rows
    per = (mt[rows] * (pt[rows] - et[rows]) ** 2).sum(1) / mt[rows].sum(1)
    L = (wt[rows] * per).sum() / B
    L.backward()
    return float(L.detach()), pt.grad.numpy(), per.detach().numpy()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,n", [(1, 4), (5, 36), (3, 1028)])
def test_specification_matches_float64_autograd(B, n, masked, weighted):
    p, e, m, t, w = _case(B, n, masked, weighted, 7 * B + n)
    got = R.weighted_mse(p, e, m, t, w)
    L, g, per = _autograd(p, e, m, t, w)
    assert abs(float(got["loss"]) - L) <= 1e-6 * abs(L)
    for b in range(B):
        err, ref = np.linalg.norm(got["grad"][b].astype(np.float64) - g[b]), np.linalg.norm(g[b])
        assert err <= 1e-6 * ref, (b, err, ref)
        assert abs(float(got["sample_loss"][b]) - per[b]) <= 1e-6 * per[b]


def test_row_without_mask_contributes_nothing():
    p, e, m, t, w = _case(4, 16, True, True, 3)
    m[2] = 0.0
    p[2, 5] = np.inf  # (whatever the row holds)
    got = R.weighted_mse(p, e, m, t, w, hist=np.zeros((7, 2)), T=T)
    assert not got["live"][2] and got["sample_loss"][2] == 0.0 and not got["grad"][2].any()
    assert np.isfinite(got["grad"]).all() and np.isfinite(got["loss"])
    p[2, 5] = 0.0
    L, g, _ = _autograd(p, e, m, t, w, rows=[0, 1, 3])  # the mean still divides by B = 4
    assert abs(float(got["loss"]) - L) <= 1e-6 * abs(L)
    assert int(got["hist"][:, 1].sum()) == 3


def test_nan_and_inf_propagate_by_plain_arithmetic():
    p, e, m, t, w = _case(3, 8, False, False, 5)
    p[1, 3] = np.nan
    got = R.weighted_mse(p, e, m, t, w)
    assert np.isnan(got["sample_loss"][1]) and np.isnan(got["loss"]) and np.isnan(got["grad"][1, 3])
    assert np.isfinite(got["grad"][[0, 2]]).all() and np.isfinite(got["sample_loss"][[0, 2]]).all()


@pytest.mark.parametrize("nbins", [1, 7, 20, 1000])
def test_histogram_bin_edges(nbins):
    """t = 0 falls in bin 0, t = T - 1 in the last bin, and a t exactly on an edge (the smallest t with (t * nbins) // T == k) opens
    bin k while its predecessor still belongs to bin k - 1."""
    assert R.bin_of(0, nbins, T) == 0 and R.bin_of(T - 1, nbins, T) == nbins - 1
    for k in range(1, nbins):
        edge = -((-k * T) // nbins)  # ceil(k T / nbins)
        assert R.bin_of(edge, nbins, T) == k and R.bin_of(edge - 1, nbins, T) == k - 1
    ts = [0, T - 1] + ([-((-1 * T) // nbins)] if nbins > 1 else [])
    sl = np.arange(1, len(ts) + 1, dtype=np.float32)
    h = R.hist_update(np.zeros((nbins, 2)), sl, np.ones(len(ts), bool), ts, T)
    assert h[:, 1].sum() == len(ts)
    for b, tb in enumerate(ts):
        assert h[R.bin_of(tb, nbins, T), 0] >= sl[b]


def test_histogram_accumulates_in_sample_order():
    sl = np.array([0.1, 0.2, 0.3, 0.7], np.float32)
    live = np.array([True, False, True, True])
    h = R.hist_update(np.zeros((2, 2)), sl, live, [10, 20, 30, 900], T)
    h = R.hist_update(h, sl, live, [10, 20, 30, 900], T)
    a = np.float64(sl[0]) + np.float64(sl[2])
    assert h[0, 0] == (a + np.float64(sl[0])) + np.float64(sl[2]) and h[0, 1] == 4
    assert h[1, 0] == np.float64(sl[3]) + np.float64(sl[3]) and h[1, 1] == 2

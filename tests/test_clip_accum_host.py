"""Gradient clipping and accumulation, the parts that need no GPU: the host specification (tests/_clip_ref.py) against
``torch.nn.utils.clip_grad_norm_`` on the CPU, and the three new entry points in the header-derived binding and in the built
library."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _clip_ref as R
from worddiffusion_amd import _native as N

SIZES = [1, 8191, 8192, 8193, 3 * 8192 + 5, 7]


def _grads(seed, scales):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * s for n, s in zip(SIZES, scales)]


@pytest.mark.parametrize("frac", [0.5, 0.03, 10.0, float("inf")])
@pytest.mark.parametrize("scales", [(1.0,) * 6, (1e-4, 1e-2, 1.0, 10.0, 1e2, 1e3)], ids=["flat", "spread"])
def test_clip_ref_against_torch_clip_grad_norm(frac, scales):
    """``max_norm = frac * norm``: clipped (0.5, 0.03), not clipped (10), measured only (inf).  torch sums in fp32 (the norm of the
    per-tensor norms), the specification in float64: 1e-6 relative on the norm and on every scaled gradient."""
    grads = _grads(3, scales)
    norm = R.global_norm(grads)
    max_norm = frac * float(norm)
    _, coef, want = R.clipped(grads, max_norm)
    params = [torch.nn.Parameter(torch.zeros(n)) for n in SIZES]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    got_norm = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    assert abs(float(got_norm) - float(norm)) <= 1e-6 * float(norm)
    assert (coef == np.float32(1.0)) == (frac >= 1.0)
    for p, w, g in zip(params, want, grads):
        d = np.abs(p.grad.numpy().astype(np.float64) - w.astype(np.float64))
        assert (d <= 1e-6 * np.abs(w.astype(np.float64))).all()
        if frac >= 1.0:
            assert np.array_equal(w, g.numpy())  # coefficient exactly 1: the gradients pass unchanged


def test_clip_ref_norm_is_the_float64_norm_rounded_once():
    grads = _grads(5, (1e-4, 1e-2, 1.0, 10.0, 1e2, 1e3)) + [None]
    exact = np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))
    norm = R.global_norm(grads)
    assert norm.dtype == np.float32 and norm == np.float32(exact)


def test_clip_coef_edges():
    one = np.float32(1.0)
    assert R.clip_coef(np.float32(3.0), float("inf")) == one
    assert R.clip_coef(np.float32(0.0), 1.0) == one               # 1 / 1e-6 clamps to 1
    assert R.clip_coef(np.float32(2.0), 1.0) == np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6))
    assert R.clip_coef(np.float32("inf"), 1.0) == np.float32(0.0)  # torch: an inf norm zeroes the finite gradients
    assert np.isnan(R.clip_coef(np.float32("nan"), 1.0))           # and a NaN norm poisons them (torch.clamp keeps NaN)
    assert np.isnan(R.clip_coef(np.float32("inf"), float("inf")))
    for norm, mx in ((float("nan"), 1.0), (float("inf"), 1.0), (float("inf"), float("inf")), (2.0, 1.0)):
        t = torch.clamp(torch.tensor(mx, dtype=torch.float32) / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0)
        r = R.clip_coef(np.float32(norm), mx)
        assert (np.isnan(r) and bool(torch.isnan(t))) or r == t.numpy()


def test_new_entry_points_are_declared_and_exported():
    v, i, i64, f, d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
    adamw = [v, i, i64, d, d, d, d, d, i64, i, d]
    assert N._SIGS["wd_adamw_multi"] == (i, adamw + [v])
    assert N._SIGS["wd_adamw_multi_scaled"] == (i, adamw + [v, v])          # ... + const float* gscale, void* stream
    assert N._SIGS["wd_grad_sqnorm_multi"] == (i, [v, i, i64, v, f, v, v])  # table, ntensor, chunks, partial, max_norm, ctl, stream
    assert N._SIGS["wd_grad_accumulate"] == (i, [v, v, i64, i, f, v])       # dst, src, n, overwrite, scale, stream
    lib = N.lib()
    for name in ("wd_adamw_multi", "wd_adamw_multi_scaled", "wd_grad_sqnorm_multi", "wd_grad_accumulate"):
        assert getattr(lib, name).argtypes == N._SIGS[name][1]
    # argument checks that launch nothing (no GPU needed): NULL pointers, a non-positive or NaN max_norm
    assert lib.wd_grad_accumulate(None, None, 4, 0, 1.0, None) == N.WD_EINVAL
    assert lib.wd_grad_sqnorm_multi(None, 1, 1, None, 1.0, None, None) == N.WD_EINVAL
    assert lib.wd_adamw_multi_scaled(None, 1, 1, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1, 0, 0.995, None, None) == N.WD_EINVAL

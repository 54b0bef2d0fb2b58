"""The whole forward on both sides of every batch size at which its launch plan changes (FULL config, 8 x 32 latents, 10 context
tokens; phosc: plus the 769-int PHOSC vector).

The planner counts 64-row panels and tiles and ``wd_gemm`` picks its tile and K cut from the grid, so the plan of B differs from
that of B - 1 at the batch sizes THRESHOLDS lists.  They are not derived here: tools/plan_thresholds.py scanned B = 1..260 (base) and
1..130 (phosc) into profiles/plan_thresholds_<variant>.txt, and tests/test_plan_thresholds_host.py holds the tables below to those
files.  At a threshold a form is first legal with the smallest grid it will ever see, or is dropped again; the kernels are tested
one by one elsewhere, what is tested here is the planner handing them the right operands at b - 1 and at b.

Reference: ``UNetOracle`` in float64 over one pool of distinct samples per variant, computed once per module in chunks of 32; a case
uses the first B samples.  The bars are the ones ``test_full_size_properties_b64`` sets: per-sample max_rel < 1e-4 against the oracle,
< 5e-5 between two batch sizes."""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests._common import FULL, make_args, max_rel  # noqa: E402
from tests._plan_sig import diff, read_scan, release, signature_at  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs, synthetic_tensor  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHOSC_LEN = 769
SEED_W = 0

# the B column of profiles/plan_thresholds_<variant>.txt (scan of B = 1..260 / 1..130)
THRESHOLDS = {
    "base": (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17, 19, 21, 22, 23, 25, 29, 32, 33, 39, 48, 63, 64, 65, 97, 129, 192, 256),
    "phosc": (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17, 19, 21, 22, 23, 25, 29, 32, 33, 43, 48, 63, 64, 65, 86, 129),
}
POOL = {"base": (257, 11), "phosc": (130, 12)}  # samples of the pool, seed of synthetic_inputs
ORACLE_CHUNK = 32


def batch_sizes(variant) -> tuple:
    """b - 1 and b of every threshold; neighbours that coincide once."""
    return tuple(sorted({B for b in THRESHOLDS[variant] for B in (b - 1, b)}))


FORWARD_CASES = [(v, B) for v in THRESHOLDS for B in batch_sizes(v)]
THRESHOLD_CASES = [(v, b) for v in THRESHOLDS for b in THRESHOLDS[v]]


def scan_file(variant) -> str:
    return os.path.join(ROOT, "profiles", f"plan_thresholds_{variant}.txt")


def pool_inputs(variant) -> dict:
    n, seed = POOL[variant]
    inp = synthetic_inputs(n, seed, phosc_len=PHOSC_LEN if variant == "phosc" else 0)
    # every sample is its own: a kernel that read a neighbour's row, timestep, word or writer would not get away with it
    assert len({inp["x"][b].numpy().tobytes() for b in range(n)}) == n
    for k in ("t", "context", "y"):
        assert len({inp[k][b].numpy().tobytes() for b in range(n)}) > n // 2, k
    return inp


def oracle_pool(variant, inp, count):
    """float64 UNetOracle over the first ``count`` samples of the pool (no case reads a later one), at most ORACLE_CHUNK at a time."""
    sd = {k: torch.from_numpy(synthetic_tensor(k, s, SEED_W)).double() for k, s in U.state_dict_shapes(FULL, variant)}
    orc = U.UNetOracle(FULL, sd, variant, variant == "phosc")
    assert orc.dtype == torch.float64
    outs = []
    with torch.no_grad():
        for b0 in range(0, count, ORACLE_CHUNK):
            s = slice(b0, min(count, b0 + ORACLE_CHUNK))
            outs.append(orc(inp["x"][s], inp["t"][s], inp["context"][s], inp["y"][s], inp["phosc"][s] if variant == "phosc" else None))
    return torch.cat(outs)


class _Pools:
    """Per variant, made on first use and kept for the module: the model on the device, the pool's inputs, the oracle's outputs (``ref=True``:
    the plan test never asks for them), and the outputs of the forwards already run (B -> CPU tensor), which the cross-threshold test reads again."""

    def __init__(self):
        self._v = {}

    def get(self, variant, ref=False):
        if variant not in self._v:
            cls = UNetModel if variant == "base" else UNetModelPhosc
            m = fill_module_(cls(args=make_args(device=DEV, phosc=1 if variant == "phosc" else 0), **FULL), SEED_W).to(DEV).eval()
            self._v[variant] = dict(model=m, inp=pool_inputs(variant), outs={})
        pool = self._v[variant]
        if ref and "ref" not in pool:  # (the first case that compares with the oracle pays for the whole pool)
            count = max(batch_sizes(variant))
            t0 = time.time()
            pool["ref"] = oracle_pool(variant, pool["inp"], count)
            print(f"\n[batch thresholds] float64 oracle, {variant}: {count} samples in {time.time() - t0:.1f} s of CPU")
        return pool


@pytest.fixture(scope="module")
def pools():
    p = _Pools()
    yield p
    for v in p._v.values():
        release(v["model"].engine)


def forward(pool, variant, B, twice=False):
    """``call`` of the model on the first B samples of the pool -> the output on the CPU; the plan is released afterwards."""
    m, inp = pool["model"], pool["inp"]
    kw = dict(timesteps=inp["t"][:B].to(DEV), context=inp["context"][:B].to(DEV), y=inp["y"][:B].to(DEV))
    x = inp["x"][:B].to(DEV)
    try:
        with torch.no_grad():
            def call():
                if variant == "base":
                    return m(x, None, original_images=None, **kw)
                return m(x, inp["phosc"][:B].to(DEV), **kw)
            out = call()
            if twice:
                assert torch.equal(call(), out), "a second call returned other bits"
        return out.cpu()
    finally:
        release(m.engine)


@pytest.mark.parametrize("variant", list(THRESHOLDS))
def test_every_listed_threshold_changes_the_plan(pools, variant):
    """Plans only: the plan of b differs from that of b - 1 exactly as the scan file says, and between two listed batch sizes
    nothing changes (the plan of b_i is the plan of b_(i+1) - 1)."""
    eng = pools.get(variant)["model"].engine
    want = read_scan(scan_file(variant))
    phosc_len = PHOSC_LEN if variant == "phosc" else 0
    sig = {B: signature_at(eng, B, phosc_len) for B in batch_sizes(variant)}
    for b in THRESHOLDS[variant]:
        assert sig[b - 1] != sig[b], f"B = {b}: the plan is that of B = {b - 1}"
        assert diff(sig[b - 1], sig[b]) == want[b], f"B = {b}"
    for b, nxt in zip(THRESHOLDS[variant], THRESHOLDS[variant][1:]):
        assert sig[b] == sig[nxt - 1], f"a threshold between B = {b} and B = {nxt - 1}: {diff(sig[b], sig[nxt - 1])}"


@pytest.mark.parametrize("variant,B", FORWARD_CASES, ids=[f"{v}-{B}" for v, B in FORWARD_CASES])
def test_forward_matches_the_oracle_on_both_sides_of_a_threshold(pools, variant, B):
    pool = pools.get(variant, ref=True)
    out = forward(pool, variant, B, twice=True)
    pool["outs"][B] = out
    assert out.shape == (B, 4, 8, 32) and out.dtype == torch.float32
    assert torch.isfinite(out).all()
    errs = [max_rel(out[b], pool["ref"][b]) for b in range(B)]
    worst = max(range(B), key=errs.__getitem__)
    print(f"\n[batch thresholds] {variant} B = {B}: worst sample {worst}, max_rel {errs[worst]:.3e} against the oracle")
    assert errs[worst] < 1e-4, [(b, e) for b, e in enumerate(errs) if e >= 1e-4]


@pytest.mark.parametrize("variant,b", THRESHOLD_CASES, ids=[f"{v}-{b}" for v, b in THRESHOLD_CASES])
def test_a_sample_keeps_its_value_across_a_threshold(pools, variant, b):
    """The first b - 1 samples of the B = b run against the B = b - 1 run: when a case above fails, this says which side moved."""
    pool = pools.get(variant)
    lo, hi = (pool["outs"][B] if B in pool["outs"] else forward(pool, variant, B) for B in (b - 1, b))
    errs = [max_rel(hi[i], lo[i]) for i in range(b - 1)]
    worst = max(range(b - 1), key=errs.__getitem__)
    print(f"\n[batch thresholds] {variant} B = {b - 1} -> {b}: worst sample {worst}, max_rel {errs[worst]:.3e} between the two runs")
    assert errs[worst] < 5e-5, [(i, e) for i, e in enumerate(errs) if e >= 5e-5]

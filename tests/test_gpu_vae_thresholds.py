"""``AutoencoderKL.decode`` / ``encode`` on both sides of every batch size at which their launch plans change (tests/_vae_cases.py: a
batch sweep of a two-level config at 8 x 32 latents up to the sampling batch, a shape sweep of a four-level config at the latent
sizes tests/_shapes.py gives the UNet).

``wd_gemm`` picks tile and K cut from its grid, so the plan of B differs from that of B - 1 at the batch sizes THRESHOLDS lists.
They are not derived here: tools/plan_thresholds.py scanned them into profiles/plan_thresholds_vae_<tag>.txt, and
tests/test_vae_thresholds_host.py holds the tables to those files.  The kernels are tested one by one elsewhere; what is tested here
is the planner handing them the right operands at b - 1 and at b: gather tables, residual rows and GroupNorm statistics of samples
that do not fill whole 128-row panels, the forced 128 x 128 tile, the one-head attention, the 3- and 8-column output convolutions.

Reference: ``oracle.vae_oracle.vae_decode`` / ``tests._vae_encode_ref.vae_encode`` in float64 over one pool of distinct samples per
tag (sample b scaled by (1, 0.5, 1.5)[b % 3]), computed once per module; a case uses the first B samples.  Every comparison is per
sample - ``max_rel`` of a sample against its own reference - so a sample that received its neighbour's statistics cannot hide behind
a larger-valued one.  The bars are the project's: < 1e-4 against the reference (tests/test_gpu_vae.py, tests/test_gpu_vae_encode.py),
< 5e-5 between two batch sizes (tests/test_gpu_batch_thresholds.py).  Measured values: profiles/vae_thresholds_errors.txt."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _vae_cases as V  # noqa: E402
from tests._common import max_rel  # noqa: E402
from tests._plan_sig import diff, read_scan, release, signature_at  # noqa: E402

DEV = "cuda:0"
ORACLE_BAR = 1e-4
CROSS_BAR = 5e-5


class _Pools:
    """Per tag, made on first use and kept for the module: the model on the device, the pool's inputs, the float64 reference (``ref=True``:
    the plan test never asks for it) and the outputs of the runs already made (B -> CPU tensors), which the cross-threshold test reads again."""

    def __init__(self):
        self._t = {}

    def get(self, tag, ref=False):
        if tag not in self._t:
            m, sd = V.build_model(tag)
            self._t[tag] = dict(model=m.to(DEV).eval(), sd=sd, inp=V.pool_inputs(tag), outs={})
        pool = self._t[tag]
        if ref and "ref" not in pool:  # (the first case that compares with the reference pays for the whole pool)
            t0 = time.time()
            pool["ref"] = V.reference(tag, pool["sd"], pool["inp"])
            print(f"\n[vae thresholds] float64 reference, {tag}: {len(pool['inp'])} samples in {time.time() - t0:.1f} s of CPU")
        return pool


@pytest.fixture(scope="module")
def pools():
    p = _Pools()
    yield p
    for tag, v in p._t.items():
        release(engine(v["model"], tag))


def engine(model, tag):
    return model.engine if V.split(tag)[0] == "dec" else model.encoder_engine


def outputs(tag, model, x) -> tuple:
    """The maps a tag's call returns, as a tuple: (image,) of ``decode``, (mean, logvar) of ``encode``."""
    if V.split(tag)[0] == "dec":
        return (model.decode(x).sample,)
    dist = model.encode(x).latent_dist
    return dist.mean, dist.logvar


def run(pool, tag, B, twice=False) -> tuple:
    """The tag's call on the first B samples of the pool -> its maps on the CPU; the plans are released afterwards."""
    m = pool["model"]
    x = pool["inp"][:B].to(DEV)
    try:
        out = outputs(tag, m, x)
        if twice:
            assert all(torch.equal(a, b) for a, b in zip(outputs(tag, m, x), out)), "a second call returned other bits"
        return tuple(t.cpu() for t in out)
    finally:
        release(engine(m, tag))


def names(tag) -> tuple:
    return ("image",) if V.split(tag)[0] == "dec" else ("mean", "logvar")


def refs(pool, tag) -> tuple:
    return (pool["ref"],) if V.split(tag)[0] == "dec" else pool["ref"]


def out_shape(tag, B) -> tuple:
    return (B, 3, *V.image_hw(tag)) if V.split(tag)[0] == "dec" else (B, 4, *V.latent_hw(tag))


def worst(errs) -> int:
    return max(range(len(errs)), key=errs.__getitem__)


@pytest.mark.parametrize("tag", V.TAGS)
def test_every_listed_threshold_changes_the_plan(pools, tag):
    """Plans only: the plan of b differs from that of b - 1 exactly as the scan file says, and between two listed batch sizes
    nothing changes (the plan of b_i is the plan of b_(i+1) - 1).  6 x 26 latents: fused statistics at the 48 x 208 level only."""
    d, _ = V.split(tag)
    eng = engine(pools.get(tag)["model"], tag)
    want = read_scan(V.scan_file(tag))
    h, w = V.latent_hw(tag) if d == "dec" else V.image_hw(tag)
    sig = {B: signature_at(eng, B, h=h, w=w, planner=eng.plan_decode if d == "dec" else eng.plan_encode) for B in V.batch_sizes(tag)}
    th = V.THRESHOLDS[tag]
    for b in th:
        assert sig[b - 1] != sig[b], f"B = {b}: the plan is that of B = {b - 1}"
        assert diff(sig[b - 1], sig[b]) == want[b], f"B = {b}"
    for b, nxt in zip(th, th[1:]):
        assert sig[b] == sig[nxt - 1], f"a threshold between B = {b} and B = {nxt - 1}: {diff(sig[b], sig[nxt - 1])}"
    for B in V.batch_sizes(tag):  # (the added batch sizes lie where the scan found no change)
        lo = max([b for b in th if b <= B], default=None)
        assert sig[B] == sig[lo if lo is not None else th[0] - 1], f"B = {B}"
    if tag in V.STAT_LEVEL_6x26:
        for B, s in sig.items():
            stat = [what for _sec, fn, what, form in s if fn == "wd_gemm" and "stat" in form[form.index("[") + 1:-1].split()]
            assert stat and all(what.startswith(V.STAT_LEVEL_6x26[tag]) for what in stat), (B, stat)


@pytest.mark.parametrize("tag,B", V.ORACLE_CASES, ids=[f"{t}-{B}" for t, B in V.ORACLE_CASES])
def test_matches_the_reference_on_both_sides_of_a_threshold(pools, tag, B):
    pool = pools.get(tag, ref=True)
    out = run(pool, tag, B, twice=True)
    pool["outs"][B] = out
    for name, o, r in zip(names(tag), out, refs(pool, tag)):
        assert o.shape == out_shape(tag, B) and o.dtype == torch.float32, name
        assert torch.isfinite(o).all(), name
        errs = [max_rel(o[b], r[b]) for b in range(B)]
        k = worst(errs)
        print(f"\n[vae thresholds] {tag} B = {B} {name}: worst sample {k}, max_rel {errs[k]:.3e} against the reference")
        assert errs[k] < ORACLE_BAR, (name, [(b, e) for b, e in enumerate(errs) if e >= ORACLE_BAR])


@pytest.mark.parametrize("tag,b", V.THRESHOLD_CASES, ids=[f"{t}-{b}" for t, b in V.THRESHOLD_CASES])
def test_a_sample_keeps_its_value_across_a_threshold(pools, tag, b):
    """The first b - 1 samples of the run at b against the run at b - 1: when a case above fails, this says which side moved."""
    pool = pools.get(tag)
    lo, hi = (pool["outs"][B] if B in pool["outs"] else run(pool, tag, B) for B in (b - 1, b))
    for name, l, h in zip(names(tag), lo, hi):
        errs = [max_rel(h[i], l[i]) for i in range(b - 1)]
        k = worst(errs)
        print(f"\n[vae thresholds] {tag} B = {b - 1} -> {b} {name}: worst sample {k}, max_rel {errs[k]:.3e} between the two runs")
        assert errs[k] < CROSS_BAR, (name, [(i, e) for i, e in enumerate(errs) if e >= CROSS_BAR])


def test_encode_chunking_at_the_real_chunk_size(pools):
    """35 images with the default ``encode_chunk``: 16 + 16 + 3, the full-chunk plan replayed and one plan for the remainder."""
    from worddiffusion_amd.vae import DiagonalGaussianDistribution
    tag, B = "enc_batch", 35
    m, sd = V.build_model(tag)
    m = m.to(DEV).eval()
    assert m.encode_chunk == m.ENCODE_CHUNK == V.ENCODE_CHUNK == 16
    g = torch.Generator().manual_seed(77)
    x = (torch.rand(B, 3, *V.image_hw(tag), generator=g) * 2 - 1) * torch.tensor([V.SAMPLE_SCALE[b % 3] for b in range(B)]).reshape(B, 1, 1, 1)
    assert len({x[b].numpy().tobytes() for b in range(B)}) == B
    t0 = time.time()
    ref = V.reference(tag, sd, x)
    print(f"\n[vae thresholds] float64 reference, {B} images: {time.time() - t0:.1f} s of CPU")
    eng = m.encoder_engine
    try:
        xd = x.to(DEV)
        dist = m.encode(xd).latent_dist
        assert len(eng._plans) == 2 and sorted(k[1] for k in eng._plans) == [3, 16]
        for name, o, r in zip(("mean", "logvar"), (dist.mean.cpu(), dist.logvar.cpu()), ref):
            assert o.shape == (B, 4, *V.latent_hw(tag)) and torch.isfinite(o).all(), name
            errs = [max_rel(o[b], r[b]) for b in range(B)]
            k = worst(errs)
            print(f"\n[vae thresholds] {tag} B = {B} (16 + 16 + 3) {name}: worst sample {k}, max_rel {errs[k]:.3e} against the reference")
            assert errs[k] < ORACLE_BAR, (name, [(b, e) for b, e in enumerate(errs) if e >= ORACLE_BAR])
        seed, off, sf = 21, 5, float(m.config.scaling_factor)
        lat = m.encode_latents(xd, seed=seed, sample_offset=off)
        whole = DiagonalGaussianDistribution(dist.mean, dist.logvar).sample(seed=seed, sample_offset=off, scale=sf)
        assert torch.equal(lat, whole)
        assert len(eng._plans) == 2
    finally:
        release(eng)

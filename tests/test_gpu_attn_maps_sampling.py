"""The samplers' ``attention=``: ``last_attention`` is the weighted mean of the per-step maps, accumulated on the device inside the
captured step (wd_xattn_maps, accumulate form).  SMALL, T = 8, n = 3.

Bit-for-bit claims.  The device adds ``w * m`` to an fp32 accumulator with two roundings, so a host fp32 sum, in step order, of the
maps of single steps must reproduce it exactly.  The single-step maps come from two replays:
  * ``forward(return_attention=True)`` on every recorded x.  A forward evaluates the time MLP inside the step, which is what the
    samplers do with ``tabulate_film = False``; against the tabulated FiLM rows (the samplers' default) the two paths agree to
    rounding only (tests/test_gpu_ddim.py holds them to 1e-5), so this replay is bit-exact for the per-step path and is held to
    the kernel bound (2e-5, tests/test_gpu_xattn_maps.py) for the default path;
  * the same sampler call with a window that selects one step (weight 1: the accumulator is that step's map, exactly), which is
    bit-exact for the default path as well.
Graph replay == eager launches, and the final x is the x of the same call without ``attention`` (SMALL never plans the one-launch
SpatialTransformer), bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _xmap_ref as X  # noqa: E402
from tests._common import SMALL, make_args, max_rel  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd.diffusion import label_padding  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

DEV = "cuda:0"
HW = (32, 64)
T, N = 8, 3
KEYS = ("input", "middle", "output")
SHAPES = {"input": (N, 4, 8, 10), "middle": (N, 2, 4, 10), "output": (N, 4, 8, 10)}
WORD = "Moving"
LABELS = torch.tensor([1, 7, 10], dtype=torch.int64)


@pytest.fixture(scope="module")
def model():
    return fill_module_(UNetModel(args=make_args(device=DEV), **SMALL), 9).to(DEV).eval()


def _x_T():
    return torch.randn(N, 4, 4, 8, generator=torch.Generator().manual_seed(3))


def _run(diff, model, sampler, attention=None, **kw):
    args = make_args(device=DEV)
    if sampler == "ddpm":
        x = diff.sampling(model, None, N, WORD, LABELS, args, x_T=_x_T(), seed=4, attention=attention, **kw)
    elif sampler == "ddim":
        x = diff.sampling_ddim(model, None, N, WORD, LABELS, args, steps=4, eta=0.5, x_T=_x_T(), seed=4, attention=attention, **kw)
    else:
        x = diff.sampling_dpmpp(model, None, N, WORD, LABELS, args, steps=4, x_T=_x_T(), seed=4, attention=attention, **kw)
    att = None if diff.last_attention is None else {k: v.cpu().numpy() for k, v in diff.last_attention.items()}
    return x.cpu(), att


def _timesteps(diff, sampler):
    return list(range(T - 1, 0, -1)) if sampler == "ddpm" else \
        diff.ddim_timesteps(4) if sampler == "ddim" else diff.dpmpp_timesteps(4)


def _host_sum(per_step, n_sel):
    w = np.float32(1.0) / np.float32(n_sel)
    acc = {k: np.zeros(SHAPES[k], dtype=np.float32) for k in KEYS}
    for m in per_step:
        for k in KEYS:
            acc[k] = X.accumulate_fp32(acc[k], w, m[k])
    return acc


def _forward_maps(model, x, t):
    ctx = torch.tensor([label_padding(WORD)] * N, dtype=torch.int64)
    with torch.no_grad():
        out = model(x.to(DEV), None, original_images=None, timesteps=torch.full((N,), t, dtype=torch.int64, device=DEV),
                    context=ctx.to(DEV), y=LABELS.to(DEV), return_attention=True)
    return {k: v.cpu().numpy() for k, v in zip(KEYS, out[1:])}


@pytest.mark.parametrize("sampler", ["ddpm", "ddim", "dpmpp"])
@pytest.mark.parametrize("window", [True, (5, 2)], ids=["all", "window"])
def test_last_attention_is_the_host_sum_of_the_steps_maps(model, sampler, window):
    diff = Diffusion(noise_steps=T, img_size=HW, args=make_args(device=DEV))
    ts = _timesteps(diff, sampler)
    sel = [t for t in ts if window is True or window[1] <= t <= window[0]]
    assert len(sel) >= 2
    plain, none = _run(diff, model, sampler)
    assert none is None and "attention_steps" not in diff.last_stats
    # ---- the default (tabulated FiLM) path: graph, eager, and the same x as without attention
    xg, ag = _run(diff, model, sampler, window)
    assert diff.last_stats["graph"] and diff.last_stats["attention_steps"] == len(sel)
    rec = []
    xe, ae = _run(diff, model, sampler, window, record=rec)
    assert not diff.last_stats["graph"] and len(rec) == len(ts)
    assert torch.equal(xg, plain) and torch.equal(xe, plain)
    for k in KEYS:
        assert ag[k].shape == SHAPES[k] and ag[k].dtype == np.float32
        assert np.array_equal(ag[k].view(np.int32), ae[k].view(np.int32)), f"{k}: graph != eager"
        assert float(np.abs(ag[k].astype(np.float64).sum(-1) - SMALL["num_heads"]).max()) < 1e-5  # a mean of maps is a map
    # single-step windows (weight 1), summed on the host in step order
    singles = [_run(diff, model, sampler, (t, t))[1] for t in sel]
    assert diff.last_stats["attention_steps"] == 1
    want = _host_sum(singles, len(sel))
    for k in KEYS:
        assert np.array_equal(ag[k].view(np.int32), want[k].view(np.int32)), f"{k}: not the two-rounding sum of the steps' maps"
    # each single step is what a forward on that step's x reports, to the kernel bound (the FiLM rows differ by rounding)
    fwd = [_forward_maps(model, rec[ts.index(t)], t) for t in sel]
    for s, f in zip(singles, fwd):
        for k in KEYS:
            assert max_rel(s[k], f[k]) < 2e-5
    # ---- the per-step FiLM path: bit for bit the host sum of forward(return_attention=True) on the recorded x
    diff.tabulate_film = False
    rec2 = []
    x2, a2 = _run(diff, model, sampler, window, record=rec2)
    x2g, a2g = _run(diff, model, sampler, window)
    assert torch.equal(x2, x2g) and torch.equal(x2, _run(diff, model, sampler)[0])
    want2 = _host_sum([_forward_maps(model, rec2[ts.index(t)], t) for t in sel], len(sel))
    for k in KEYS:
        assert np.array_equal(a2[k].view(np.int32), want2[k].view(np.int32)), f"{k}: not the host sum of the forwards' maps"
        assert np.array_equal(a2[k].view(np.int32), a2g[k].view(np.int32)), f"{k}: graph != eager (per-step FiLM)"


def test_sampling3_skipped_steps_add_nothing(model):
    T3 = 12
    diff = Diffusion(noise_steps=T3, img_size=HW, args=make_args(device=DEV))
    args = make_args(device=DEV)
    x_T = torch.randn(N, 4, 4, 8, generator=torch.Generator().manual_seed(5))
    words = [WORD] * N

    def run(attention=None, **kw):
        x = diff.sampling3(0, None, words, None, model, model, None, 0, 1, N, WORD, LABELS, args, seed=2, x_T=x_T,
                           attention=attention, **kw)
        return x.cpu(), (None if diff.last_attention is None else {k: v.cpu().numpy() for k, v in diff.last_attention.items()})

    calls = [i for i in range(T3 - 1, 0, -1) if Diffusion.sampling3_calls_model(i, T3, 0)]
    assert calls == [11, 10, 5]
    plain, _ = run()
    xg, ag = run(True)
    assert diff.last_stats["attention_steps"] == len(calls) == diff.last_stats["model_calls"] and diff.last_stats["graph"]
    assert torch.equal(xg, plain)
    xe, ae = run(True, use_graph=False)
    singles = [run((t, t))[1] for t in calls]
    want = _host_sum(singles, len(calls))
    for k in KEYS:
        assert np.array_equal(ag[k].view(np.int32), ae[k].view(np.int32))
        assert np.array_equal(ag[k].view(np.int32), want[k].view(np.int32)), k  # 8 of the 11 steps ran no forward and added nothing
    with pytest.raises(ValueError):
        run((9, 6))  # visited, but no step in it calls the model
    assert diff.last_stats["attention_steps"] == 1  # (of the last successful call: the rejected one launched nothing)


def test_rejections_happen_on_the_host(model):
    diff = Diffusion(noise_steps=T, img_size=HW, args=make_args(device=DEV))
    args = make_args(device=DEV)
    with pytest.raises(ValueError):
        diff.sampling(model, None, N, WORD, LABELS, args, attention=(0, 0))
    with pytest.raises(ValueError):
        diff.sampling_ddim(model, None, N, WORD, LABELS, args, steps=4, attention=(2, 5))
    pargs = make_args(device=DEV, phosc=1)
    mp = fill_module_(UNetModelPhosc(args=pargs, **SMALL), 2).to(DEV).eval()
    ph = torch.randint(0, 2, (N, 12), generator=torch.Generator().manual_seed(1))
    with pytest.raises(NotImplementedError):
        diff.sampling(mp, None, N, WORD, LABELS, pargs, phoscLabels=ph, attention=True)
    assert mp._engine is None or not mp.engine._plans


def test_driver_regenerate_saves_the_maps_beside_the_images(model, tmp_path):
    from worddiffusion_amd.driver import regenerate
    args = make_args(device=DEV)
    diff = Diffusion(noise_steps=T, img_size=HW, args=args)
    rows = [("w1", "img_a", "Moving"), ("w7", "img_b", "ab"), ("w1", "img_c", "word")]
    wr = {"w1": 1, "w7": 7}
    out_dir = str(tmp_path / "images")
    regenerate(model, diff, rows, wr, args, batch=2, out_dir=out_dir, seed=6, rank=0, world=1, sampler="ddim", ddim_steps=4,
               attention=(5, 2), attn_out="maps.npz")
    z = np.load(tmp_path / "images" / "maps.npz")
    assert [str(v) for v in z["images"]] == ["img_a", "img_b", "img_c"] and [str(v) for v in z["words"]] == ["Moving", "ab", "word"]
    assert z["input"].shape == (3, 4, 8, 10) and z["middle"].shape == (3, 2, 4, 10) and z["output"].shape == (3, 4, 8, 10)
    x = diff.sampling_ddim(model, None, 2, ["Moving", "ab"], torch.tensor([1, 7]), args, steps=4, seed=6, attention=(5, 2))
    for k in KEYS:
        assert np.array_equal(z[k][:2], diff.last_attention[k].cpu().numpy())
    assert np.array_equal(np.load(tmp_path / "images" / "img_b.npy"), x[1].cpu().numpy())

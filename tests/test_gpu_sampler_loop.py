"""The reverse loop's exits (``Diffusion._denoise`` / ``_sample``): a call that raises on the host mid-loop leaves no captured graph
behind and the objects usable, and a refused call has launched nothing and drawn nothing from ``random``.  Every failing call
here raises an ordinary Python exception on the host.  The library is watched through a recording proxy in place of ``_native.lib``."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import SMALL, make_args  # noqa: E402
from worddiffusion_amd import Diffusion, UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

DEV, HW, n = "cuda:0", (32, 64), 2


class Recorder:
    """Stands in for the library: (name, return value) of every entry point called through it, in order."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            rc = fn(*a)
            self.calls.append((name, rc))
            return rc
        call.__name__ = name
        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder(N.lib())
    monkeypatch.setattr(N, "lib", lambda: rec)
    return rec


def _pair(T, cls=UNetModel, cfg=SMALL, seed=5, **args_kw):
    args = make_args(device=DEV, **args_kw)
    return Diffusion(noise_steps=T, img_size=HW, args=args), fill_module_(cls(args=args, **cfg), seed).to(DEV).eval(), args


def _graphs(rec):
    ended = sum(1 for name, rc in rec.calls if name == "wd_graph_end" and rc == 0)
    return ended, sum(1 for name, _ in rec.calls if name == "wd_graph_destroy")


def test_a_call_that_raises_mid_loop_leaves_no_graph_behind(recorder):
    T = 6
    labels = torch.tensor([1, 2], dtype=torch.int64)
    short = [torch.zeros(n, 4, 4, 8) for _ in range(T - 3)]  # t = 5 .. 2 read entries 0 .. 3: one short
    diff, m, args = _pair(T)
    with pytest.raises(IndexError):
        diff.sampling(m, None, n, "MOVE", labels, args, noise=short, seed=3, use_graph=True)
    assert _graphs(recorder) == (1, 1)
    assert m.training  # train.py:238, on this exit too
    after = diff.sampling(m, None, n, "MOVE", labels, args, seed=3)
    fresh_diff, fresh_m, _ = _pair(T)
    assert torch.equal(after, fresh_diff.sampling(fresh_m, None, n, "MOVE", labels, args, seed=3))
    assert _graphs(recorder) == (3, 3)
    # sampling3 at T = 6 calls the model at t = 5 alone, so it captures the whole step and the tail alone: both go
    del recorder.calls[:]

    def bulk(d, mm, **kw):
        return d.sampling3(0, None, ["MOVE"] * n, None, mm, mm, None, 0, 1, n, "MOVE", labels, args, seed=3, **kw)
    with pytest.raises(IndexError):
        bulk(diff, m, noise=short)
    assert _graphs(recorder) == (2, 2)
    after = bulk(diff, m)
    assert diff.last_stats["model_calls"] == 1 and diff.last_stats["graph"]
    assert torch.equal(after, bulk(fresh_diff, fresh_m))
    assert _graphs(recorder) == (6, 6)


@pytest.mark.parametrize("which, extra", [("sampling", {}), ("sampling_ddim", dict(steps=3)), ("sampling_dpmpp", dict(steps=3))])
def test_a_refused_call_launches_nothing_and_draws_nothing(recorder, which, extra):
    diff, m, args = _pair(6, UNetModelPhosc, dict(SMALL, num_classes=339), 9, interpolation=True)
    labels = torch.tensor([1, 2], dtype=torch.int64)
    refused = [(dict(mix_rate=0.37, guidance="text_free"), "guidance must be"),
               (dict(mix_rate=0.37, guidance="writer_free"), "interpolation"),
               (dict(mix_rate=torch.tensor([0.1, 0.2, 0.3])), "mix_rate must be"),
               (dict(mix_rate=0.37, style_pairs=(1, 2, 3)), "style_pairs must be")]
    random.seed(17)
    state = random.getstate()
    del recorder.calls[:]  # (whatever building the model called)
    for kw, message in refused:
        with pytest.raises(ValueError, match=message):
            getattr(diff, which)(m, None, n, "MOVE", labels, args, seed=3, **extra, **kw)
        assert random.getstate() == state, kw
        assert recorder.calls == [], kw
    assert diff.last_stats == {}

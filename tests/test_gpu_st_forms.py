"""Which launches a SpatialTransformer of the 8 x 32 level gets under each transformer switch, and that ``UNetEngine._st_form``
names that form.  FULL base model; plans are built, nothing but ``refresh_weights`` is launched.  The launch lists are the ones
the planner produced before it was split into one method per form (recorded with tools/plan_dump.py), not derived from
``_st_form``.  B = 48 is the smallest batch whose 8 x 32 level has the 192 panels the fused feed-forward waits for; the one-launch
form also needs proj_in to apply the GroupNorm itself (256 panels), so it is checked at B = 64."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests._common import FULL, make_args  # noqa: E402
from worddiffusion_amd import UNetModel  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_  # noqa: E402

DEV = "cuda:0"
PROJ_IN_48 = ["wd_gn_apply", "wd_gemm"]  # (B = 48: GroupNorm planes, then proj_in; B = 64: proj_in applies the norm itself)
PLAIN_ATTN = ["wd_layernorm", "wd_gemm", "wd_attention", "wd_gemm"]
MID_TAPPED = ["wd_gemm", "wd_xattn_planes", "wd_xattn_maps", "wd_gemm", "wd_gemm"]  # (4 x 16: 64 panels, the two-source tail)

# (environment, B) -> launches of in1.1, its (form, tail)
CASES = {
    "default": ({}, 48, PROJ_IN_48 + ["wd_xattn_pair", "wd_ff_fused"], ("pair", "ff+proj")),
    "FUSE_ST=0": ({"WDIFF_FUSE_ST": "0"}, 48, PROJ_IN_48 + ["wd_xattn_pair", "wd_ff_fused"], ("pair", "ff+proj")),
    "FUSE_XATTN_PAIR=0": ({"WDIFF_FUSE_XATTN_PAIR": "0"}, 48, PROJ_IN_48 + ["wd_xattn_fused", "wd_xattn_fused", "wd_ff_fused"],
                          ("folded", "ff+proj")),
    "FUSE_XATTN=0": ({"WDIFF_FUSE_XATTN": "0"}, 48, PROJ_IN_48 + PLAIN_ATTN + PLAIN_ATTN + ["wd_layernorm", "wd_ff_fused"],
                     ("plain", "ff+proj")),
    "FUSE_FF=0": ({"WDIFF_FUSE_FF": "0"}, 48, PROJ_IN_48 + ["wd_xattn_planes", "wd_gemm", "wd_gemm"], ("pair", "two-source")),
    "FUSE_PROJ=0": ({"WDIFF_FUSE_PROJ": "0"}, 48, PROJ_IN_48 + ["wd_xattn_pair", "wd_ff_fused", "wd_gemm"], ("pair", "proj_out")),
    "FOLD_PROJ=0": ({"WDIFF_FOLD_PROJ": "0"}, 48, PROJ_IN_48 + ["wd_xattn_pair", "wd_ff_fused"], ("pair", "ff+proj")),
    "FUSE_FF=0 FOLD_PROJ=1": ({"WDIFF_FUSE_FF": "0", "WDIFF_FOLD_PROJ": "1"}, 48,
                              PROJ_IN_48 + ["wd_xattn_planes", "wd_gemm", "wd_gemm"], ("pair", "two-source")),
    "default, B = 64": ({}, 64, ["wd_ff_fused"], ("one-launch", "ff+proj")),
    "FUSE_ST=0, B = 64": ({"WDIFF_FUSE_ST": "0"}, 64, ["wd_gemm", "wd_xattn_pair", "wd_ff_fused"], ("pair", "ff+proj")),
}


def _plan(monkeypatch, env, B, **kw):
    """A fresh FULL base model under ``env`` -> (launches per SpatialTransformer name, what _st_form said per name)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = fill_module_(UNetModel(args=make_args(device=DEV), **FULL), 1).to(DEV).eval()
    eng = m.engine
    forms, st_form = {}, eng._st_form

    def recording(P, name, mod, x):
        forms[name] = st_form(P, name, mod, x)
        return forms[name]

    monkeypatch.setattr(eng, "_st_form", recording)
    eng.refresh_weights()
    P = eng.plan(B, 8, 32, 10, 0, **kw)
    launches = {name: [fn.__name__ for fn, _, what in P.step if what.startswith((name + ".", name + ":"))] for name in forms}
    del P, eng, m
    gc.collect()  # (model and engine refer to each other; a B = 48 plan holds close to 1 GB)
    torch.cuda.empty_cache()
    return launches, forms


@pytest.mark.parametrize("case", list(CASES))
def test_first_8x32_transformer_under_each_switch(monkeypatch, case):
    env, B, want, (form, tail) = CASES[case]
    launches, forms = _plan(monkeypatch, env, B)
    assert list(forms) == ["in1.1", "mid.1", "out2.1", "out3.1"]
    f = forms["in1.1"]
    assert (f.B, f.h, f.w, f.c, f.hw, f.M, f.heads, f.d, f.inner, f.L) == (B, 8, 32, 320, 256, B * 256, 4, 80, 320, 10)
    assert launches["in1.1"] == want
    assert (f.form, f.tail) == (form, tail)
    assert f.gn_in == (B == 64) and not f.tap
    assert f.xfold == ("WDIFF_FUSE_XATTN" not in env)


@pytest.mark.parametrize("B", [48, 64])
def test_attention_maps_tap_three_blocks_and_leave_the_fourth(monkeypatch, B):
    """The tapped blocks (in1.1, mid.1, out3.1) take the chain plus one wd_xattn_maps behind the attention launch; out2.1 keeps the
    form the default plan gives it - the one launch at B = 64."""
    launches, forms = _plan(monkeypatch, {}, B, attn_maps=True)
    proj_in = PROJ_IN_48 if B == 48 else ["wd_gemm"]
    tapped = proj_in + ["wd_xattn_pair", "wd_xattn_maps", "wd_ff_fused"]
    assert launches["in1.1"] == tapped and launches["out3.1"] == tapped
    assert launches["mid.1"] == MID_TAPPED
    assert launches["out2.1"] == (proj_in + ["wd_xattn_pair", "wd_ff_fused"] if B == 48 else ["wd_ff_fused"])
    assert [forms[n].tap for n in ("in1.1", "mid.1", "out2.1", "out3.1")] == [True, True, False, True]
    assert [forms[n].form for n in ("in1.1", "mid.1", "out3.1")] == ["pair"] * 3
    assert forms["mid.1"].tail == "two-source" and forms["in1.1"].tail == "ff+proj"
    assert forms["out2.1"].form == ("pair" if B == 48 else "one-launch")

"""Host side of the batch-threshold tests: the tables of tests/test_gpu_batch_thresholds.py are the batch sizes the committed scans
list (profiles/plan_thresholds_<variant>.txt, written by tools/plan_thresholds.py), every one of them is run on both sides, and
``signature`` / ``diff`` of tests/_plan_sig.py say what they should on two small hand-made op lists (nothing is launched: the
library only answers wd_gemm_check).  The same for the training step: the tables of tests/test_gpu_train_thresholds.py against
profiles/plan_thresholds_train_<variant>.txt, and ``train_signature`` on a hand-made backward list (wd_dw_slices and
wd_dw_group_slices are host functions)."""
import ctypes
import types

import pytest

from tests import test_gpu_batch_thresholds as G
from tests import test_gpu_train_thresholds as GT
from tests._plan_sig import diff, read_scan, signature, train_signature
from worddiffusion_amd import _native as N

SCANNED_TO = {"base": 260, "phosc": 130}  # the top of each committed scan
_P = 1 << 20  # placeholder operand address: non-NULL, 16-byte aligned (wd_gemm_check reads no memory)


@pytest.mark.parametrize("variant", sorted(SCANNED_TO))
def test_the_gpu_tables_are_the_committed_scans(variant):
    with open(G.scan_file(variant)) as f:
        head = f.readline()
    assert head.startswith("#") and f"FULL {variant}," in head and f"B = 1..{SCANNED_TO[variant]};" in head, head
    scan = read_scan(G.scan_file(variant))
    assert list(scan) == sorted(scan) and min(scan) >= 2 and max(scan) <= SCANNED_TO[variant]
    assert G.THRESHOLDS[variant] == tuple(scan), "re-run tools/plan_thresholds.py and copy its B column into THRESHOLDS"
    assert max(scan) <= G.POOL[variant][0], "the pool has too few samples for the largest threshold"


@pytest.mark.parametrize("variant", sorted(SCANNED_TO))
def test_no_threshold_is_dropped_from_the_cases(variant):
    """Every listed b is a case of the cross-threshold test, and b - 1 and b are both cases of the oracle test, each once."""
    scan = read_scan(G.scan_file(variant))
    assert [b for v, b in G.THRESHOLD_CASES if v == variant] == list(scan)
    ran = [B for v, B in G.FORWARD_CASES if v == variant]
    assert len(ran) == len(set(ran)) and set(ran) == {B for b in scan for B in (b - 1, b)}
    names = {f.__name__: f for f in (G.test_forward_matches_the_oracle_on_both_sides_of_a_threshold,
                                     G.test_a_sample_keeps_its_value_across_a_threshold)}
    for name, cases in (("test_forward_matches_the_oracle_on_both_sides_of_a_threshold", G.FORWARD_CASES),
                        ("test_a_sample_keeps_its_value_across_a_threshold", G.THRESHOLD_CASES)):
        marks = [mk for mk in names[name].pytestmark if mk.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == cases, name
    assert all(mk.name != "skip" and mk.name != "xfail" for f in names.values() for mk in f.pytestmark)


def test_the_issue_table_is_in_the_base_scan():
    """The batch sizes reading the planner's rules suggests (the 64 x 80 whole-K window 32..128, wd_ff_fused at 192 panels, the
    weights-to-registers kernel at 256 tiles) are among those the scan found."""
    scan = read_scan(G.scan_file("base"))
    assert {32, 48, 64, 129, 192, 256} <= set(scan)
    assert "K_GEMMQ" in scan[32] and "K_GEMMQ" in scan[129] and "K_GEMMW" in scan[64] and "K_GEMMW" in scan[256]
    assert "+ wd_ff_fused x3" in scan[48] and "+ wd_ff_fused x1" in scan[192]


# ---- the training step's tables
@pytest.mark.parametrize("variant", sorted(GT.SCANNED_TO))
def test_the_train_tables_are_the_committed_scans(variant):
    assert GT.SCANNED_TO == {"base": 72, "phosc": 32}  # the ranges the training scans cover
    with open(GT.scan_file(variant)) as f:
        head = f.readline()
    assert head.startswith("#") and f"FULL {variant} training step," in head and f"B = 1..{GT.SCANNED_TO[variant]};" in head, head
    scan = read_scan(GT.scan_file(variant))
    assert list(scan) == sorted(scan) and min(scan) >= 2 and max(scan) <= GT.SCANNED_TO[variant]
    assert GT.THRESHOLDS[variant] == tuple(scan), "re-run tools/plan_thresholds.py --variant train-* and copy its B column into THRESHOLDS"
    assert all(text.strip() and text != "same ops in another order" for text in scan.values())


@pytest.mark.parametrize("variant", sorted(GT.SCANNED_TO))
def test_no_train_threshold_is_dropped_from_the_cases(variant):
    """Every listed b is a case of the cross-threshold test; b - 1, b and the scan's upper end are cases of the gradient test,
    each once and in ascending order (the running reference then passes over the pool once)."""
    scan = read_scan(GT.scan_file(variant))
    assert [b for v, b in GT.THRESHOLD_CASES if v == variant] == list(scan)
    ran = [B for v, B in GT.GRADIENT_CASES if v == variant]
    assert ran == sorted(set(ran)) and set(ran) == {B for b in scan for B in (b - 1, b)} | {GT.SCANNED_TO[variant]}
    names = {f.__name__: f for f in (GT.test_training_gradients_on_both_sides_of_a_threshold,
                                     GT.test_a_sample_keeps_its_prediction_across_a_threshold)}
    for name, cases in (("test_training_gradients_on_both_sides_of_a_threshold", GT.GRADIENT_CASES),
                        ("test_a_sample_keeps_its_prediction_across_a_threshold", GT.THRESHOLD_CASES)):
        marks = [mk for mk in names[name].pytestmark if mk.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == cases, name
    assert all(mk.name != "skip" and mk.name != "xfail" for f in names.values() for mk in f.pytestmark)


def test_the_train_scans_show_what_the_training_planner_decides():
    """The forms ``TrainEngine._dw_form`` and the library decide by the batch are among the differences the scans found: slice
    counts of both wd_dw forms, K cuts of data-gradient GEMMs, and at B = 32 - the first batch whose 320 word tokens fill 64-row
    units - the word encoder's weight gradients leaving transposed planes + wd_gemm for wd_dw."""
    base, phosc = read_scan(GT.scan_file("base")), read_scan(GT.scan_file("phosc"))
    for scan in (base, phosc):
        assert any("wd_dw ntaps=" in t and "slices=" in t for t in scan.values())
        assert any("wd_dw_group items=" in t for t in scan.values())
        assert any("bwd: " in t and ":dX" in t and "ksplit=" in t for t in scan.values())
    assert "bwd: cross.kv:dW0, bwd: word_emb.qkv:dW0: wd_gemm " in base[32] and "-> wd_dw ntaps=1 hw_out=64 hw_src=64" in base[32]
    assert "- wd_transpose_planes x2: bwd: cross.kv:T(x0), bwd: word_emb.qkv:T(x0)" in base[32]
    assert "+ wd_transpose_planes x2: bwd: cross.kv:T(x0), bwd: word_emb.qkv:T(x0)" in base[33]


# ---- signature / diff on hand-made op lists
def _gemm(m, n, hw_out, srcs, **fields):
    """srcs: (c, ntaps, gathered, hw_src) per source; every pointer a placeholder."""
    a = N.WdGemmArgs()
    for i, (c, ntaps, gathered, hw_src) in enumerate(srcs):
        s = a.src[i]
        s.hi = s.lo = _P
        s.gather = _P if gathered else None
        s.ld, s.c, s.ntaps, s.hw_src = c, c, ntaps, hw_src
    a.nsrc, a.npass, a.w_hi, a.w_lo = len(srcs), 3, _P, _P
    a.m, a.n, a.ktot, a.hw_out = m, n, sum(c * t for c, t, _, _ in srcs), hw_out
    a.out_f32, a.out_ld, a.ws, a.ws_floats = _P, n, _P, 128 * 128 * 160 * 8
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _ff(**fields):
    a = N.WdFfArgs()
    a.m, a.c, a.inner, a.npass = 64 * 256, 320, 1280, 3
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def _plans():
    """Two plans of four-and-a-bit ops each, as (engine, P): a 4 x 16 convolution on the K-cut kernel (B = 8) and on the 64 x 80
    whole-K kernel (B = 64), a feed-forward as GEMMs and as wd_ff_fused, and a conditioning GEMM that only grows."""
    lib = N.lib()
    eng = types.SimpleNamespace(lib=lib)
    conv = [(640, 9, True, 64)]

    def plan(B, fused):
        cond = [(lib.wd_embed_tokens, (), "word_emb.embedding"),
                (lib.wd_gemm, (ctypes.byref(_gemm(B * 10, 960, 10, [(320, 1, False, 0)], tile=128160)),), "word_emb.qkv")]
        if fused:
            step = [(lib.wd_gemm, (ctypes.byref(_gemm(B * 64, 640, 64, conv, w_layout=3, tile=64080, slab_rows=16)),), "mid.0.conv1"),
                    (lib.wd_ff_fused, (ctypes.byref(_ff(w3_hi=_P, w32_hi=_P, stat_part=_P)),), "mid.1.tb0.ff + proj_out (fused)")]
        else:
            step = [(lib.wd_gemm, (ctypes.byref(_gemm(B * 64, 640, 64, conv)),), "mid.0.conv1"),
                    (lib.wd_layernorm, (), "mid.1.tb0.norm3"),
                    (lib.wd_gemm, (ctypes.byref(_gemm(B * 64, 2560, 64, [(320, 1, False, 0)], act=N.ACT_GEGLU, tile=128160,
                                                      out_f32=None, out_hi=_P, out_lo=_P, out_pl_ld=1280)),), "mid.1.tb0.ff1")]
        return eng, types.SimpleNamespace(cond=cond, step=step, film=[(lib.wd_timestep_embedding, (), "never read")])

    return plan(8, False), plan(64, True)


CONV_CUT = "K_M16 w_layout=0 tile=128160 ksplit=16 nsrc=1 [f32]"        # 16 tiles of 128 x 160: 256 / 16 slices (90 K-steps of 64)
CONV_WHOLE_K = "K_GEMMQ w_layout=3 tile=64080 ksplit=1 nsrc=1 [slab_rows f32]"


def test_signature_of_a_hand_made_plan():
    (eng, small), (_, large) = _plans()
    qkv = ("cond", "wd_gemm", "word_emb.qkv", "K_M16 w_layout=0 tile=128160 ksplit=1 nsrc=1 [f32]")
    assert signature(eng, small) == (
        ("cond", "wd_embed_tokens", "word_emb.embedding", ""), qkv,
        ("step", "wd_gemm", "mid.0.conv1", CONV_CUT),
        ("step", "wd_layernorm", "mid.1.tb0.norm3", ""),
        ("step", "wd_gemm", "mid.1.tb0.ff1", "K_M16 w_layout=0 tile=128160 ksplit=1 nsrc=1 [planes]"))
    assert signature(eng, large) == (
        ("cond", "wd_embed_tokens", "word_emb.embedding", ""), qkv,
        ("step", "wd_gemm", "mid.0.conv1", CONV_WHOLE_K),
        ("step", "wd_ff_fused", "mid.1.tb0.ff + proj_out (fused)", "no front, proj_out folded, stat"))


def _dw(m, n, c, ntaps, hw_out, hw_src, **fields):
    a = N.WdDwArgs()
    a.d_hi = a.d_lo = a.x_hi = a.x_lo = a.grad = a.ws = _P
    a.m, a.n, a.c, a.ntaps, a.hw_out, a.hw_src, a.npass = m, n, c, ntaps, hw_out, hw_src, 3
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def test_train_signature_of_a_hand_made_backward_list():
    """cond, step and bwd, with the two wd_dw forms: the slice count is the library's for the op's (m, n, c, ntaps) - the args carry
    nslice = 0 -, no row count or address enters, and ``signature`` of the same plan is its forward part."""
    lib = N.lib()
    (eng, P), _ = _plans()
    items = (N.WdDwItem * 5)()

    def bwd(B, base):
        return [(lib.wd_dout_prep, (), "mid.0.conv1:prep(dout)"),
                (lib.wd_dw, (ctypes.byref(_dw(B * 64, 640, 640, 9, 64, 64, gather=base, grad=base + 64)),), "mid.0.conv1:dW0"),
                (lib.wd_dw_group, (ctypes.byref(_dw(B * 64, 640, 640, 1, 64, 64, ws=base)), ctypes.cast(items, ctypes.c_void_p), base, 5),
                 "dW group: a, b, c, d, e")]

    P.bwd, P.bwd_cuts, P.bwd_segments = bwd(8, _P), [(1, 0)], [(0, 1, 0, 64)]
    sig = train_signature(eng, P)
    assert sig[:len(signature(eng, P))] == signature(eng, P) and len(sig) == len(signature(eng, P)) + 3
    s9, s1g = lib.wd_dw_slices(512, 640, 640, 9), lib.wd_dw_group_slices(512, 640, 640, 1, 5)
    assert s9 >= 1 and s1g >= 1
    assert sig[-3:] == (("bwd", "wd_dout_prep", "mid.0.conv1:prep(dout)", ""),
                        ("bwd", "wd_dw", "mid.0.conv1:dW0", f"ntaps=9 hw_out=64 hw_src=64 npass=3 accumulate=0 slices={s9}"),
                        ("bwd", "wd_dw_group", "dW group: a, b, c, d, e", f"items=5 ntaps=1 hw_out=64 hw_src=64 slices={s1g}"))
    # other addresses, cuts and segments: the same signature; another batch: only what the library decides by it
    P.bwd, P.bwd_cuts, P.bwd_segments = bwd(8, _P << 4), [(2, 1)], [(0, 2, 0, 128)]
    assert train_signature(eng, P) == sig and hash(train_signature(eng, P)) == hash(sig)
    P.bwd = bwd(64, _P)
    big = train_signature(eng, P)
    t9, t1g = lib.wd_dw_slices(4096, 640, 640, 9), lib.wd_dw_group_slices(4096, 640, 640, 1, 5)
    assert (big == sig) == ((s9, s1g) == (t9, t1g))
    if t9 != s9:
        assert f"bwd: mid.0.conv1:dW0: wd_dw ntaps=9 hw_out=64 hw_src=64 npass=3 accumulate=0 slices={s9} -> wd_dw ntaps=9 hw_out=64 " \
               f"hw_src=64 npass=3 accumulate=0 slices={t9}" in diff(sig, big)


def test_signature_holds_nothing_that_only_grows_with_the_batch():
    """Other row counts and other addresses, the same forms: equal signatures (and hashable ones)."""
    lib = N.lib()
    eng = types.SimpleNamespace(lib=lib)

    def plan(B, base):
        a = _gemm(B * 256, 320, 256, [(320, 9, True, 256)], w_layout=3, tile=64320, slab_rows=32, out_f32=base, w_hi=base + 4096,
                  stat_part=base + 8192, stat_cpg=10)
        f = _ff(m=B * 256, x_in=base, tok2=base + 64, w3_hi=base + 128)
        return types.SimpleNamespace(cond=[], step=[(lib.wd_gemm, (ctypes.byref(a),), "in1.0.conv1"),
                                                    (lib.wd_ff_fused, (ctypes.byref(f),), "in1.1.tb0: fused")])

    s64, s200 = signature(eng, plan(64, 1 << 20)), signature(eng, plan(200, 1 << 30))
    assert s64 == s200 and hash(s64) == hash(s200) and diff(s64, s200) == ""
    assert s64[0][3] == "K_GEMMW w_layout=3 tile=64320 ksplit=1 nsrc=1 [slab slab_rows stat f32]"
    assert s64[1][3] == "front, proj_out, tok2 written"


def test_diff_of_two_hand_made_plans():
    (eng, small), (_, large) = _plans()
    a, b = signature(eng, small), signature(eng, large)
    assert diff(a, a) == "" and diff(b, b) == ""
    assert diff(a, b) == (f"mid.0.conv1: wd_gemm {CONV_CUT} -> wd_gemm {CONV_WHOLE_K}; - wd_layernorm x1: mid.1.tb0.norm3; "
                          "- wd_gemm x1: mid.1.tb0.ff1; + wd_ff_fused x1: mid.1.tb0.ff + proj_out (fused)")
    assert diff(b, a) == (f"mid.0.conv1: wd_gemm {CONV_WHOLE_K} -> wd_gemm {CONV_CUT}; - wd_ff_fused x1: mid.1.tb0.ff + proj_out (fused); "
                          "+ wd_layernorm x1: mid.1.tb0.norm3; + wd_gemm x1: mid.1.tb0.ff1")


def test_diff_groups_equal_changes_and_counts_past_three():
    sig = tuple(("step", "wd_gemm", f"l{i}.conv", "A") for i in range(5)) + (("cond", "wd_gemm", "kv", "A"), ("cond", "wd_gemm", "kv", "A"))
    moved = tuple((s, f, w, "B" if w != "l4.conv" else "C") for s, f, w, _ in sig[:5]) + (sig[5], ("cond", "wd_gemm", "kv", "D"))
    assert diff(sig, moved) == ("l0.conv, l1.conv, l2.conv (+1 more): wd_gemm A -> wd_gemm B; l4.conv: wd_gemm A -> wd_gemm C; "
                                "cond: kv #2: wd_gemm A -> wd_gemm D")
    assert diff(sig[:2], (sig[1], sig[0])) == "same ops in another order"


def test_read_scan_refuses_what_is_not_a_threshold_line(tmp_path):
    p = tmp_path / "scan.txt"
    p.write_text("# head\nB=3: a -> b\n\nB=7: c: d -> e; + f\n")
    assert read_scan(str(p)) == {3: "a -> b", 7: "c: d -> e; + f"}
    for bad in ("B=3 a\n", "3: a\n", "B=3: a\nB=3: b\n", "B=x: a\n"):
        p.write_text(bad)
        with pytest.raises(ValueError):
            read_scan(str(p))

"""wd_epilogue_batch_ok (csrc/wd_gemm_epi.h), the one rule that says which launches take the batched 64-row tile epilogue, asked
without a GPU: through wd_epilogue_batch_applies on resolved args, and through the dbg bit wd_gemm_check / wd_ff_check resolve
(WD_EPI_BATCH_ON / _OFF force the form on / off for a call, resolved WD_EPI_BATCH_BIT = batched form taken).  Nothing is launched.  The shapes of
the B = 64 step are stated here by hand; tests/test_gpu_epilogue_batched.py asks the same of the plan the engine really builds."""
import ctypes

import pytest

from tests.test_host_logic import _P, _PLANES, _gemm_args
from worddiffusion_amd import _native as N

ON, OFF = N.EPI_BATCH_ON, N.EPI_BATCH_OFF
_M = 64 * 256  # B = 64 samples of 8 x 32
_CONV = dict(w_layout=3, tile=64320, slab_rows=32, bias=_P)
_STAT = dict(stat_part=_P, stat_cpg=10)


def _resolve(a):
    out = N.WdGemmArgs()
    assert N.lib().wd_gemm_check(ctypes.byref(a), ctypes.byref(out)) == N.WD_OK
    return out


# name: (args with dbg = ON, does the launch take the batched form)
_TABLE = {
    # the 64 x 320 launches of the B = 64 step
    "3x3 320 -> 320, FiLM row": (_gemm_args(_M, 320, 256, [(320, 9, True, 256)], rowvec=_P, rowvec_ld=320, **_CONV, **_STAT), True),
    "3x3 320 -> 320, residual, planes": (_gemm_args(_M, 320, 256, [(320, 9, True, 256)], resid=_P, resid_ld=320, out_pl_ld=320, **_CONV,
                                                   **_STAT, **_PLANES), True),
    "3x3 640 -> 320": (_gemm_args(_M, 320, 256, [(640, 9, True, 256)], rowvec=_P, rowvec_ld=320, **_CONV, **_STAT), True),
    "3x3 320 -> 320 + 1x1 skip of 640": (_gemm_args(_M, 320, 256, [(320, 9, True, 256), (640, 1, False, 0)], **_CONV, **_STAT), True),
    "Upsample, 4 phases": (_gemm_args(_M, 320, 256, [(640, 4, True, 64)], w_layout=3, tile=64320, w_ngroups=4, w_group_stride=320 * 4 * 640,
                                      bias=_P, **_STAT), True),
    "4x16 conv, 64 x 80 plain tail": (_gemm_args(64 * 64, 640, 64, [(640, 9, True, 64)], w_layout=3, tile=64080, slab_rows=16, bias=_P), True),
    "SiLU": (_gemm_args(128, 320, 64, [(64, 1, False, 0)], w_layout=3, tile=64320, act=N.ACT_SILU), True),
    # what the predicate refuses
    "m = 96: ragged last tile": (_gemm_args(96, 320, 32, [(64, 1, False, 0)], w_layout=3, tile=64320), False),
    "hw_out = 32: two samples per panel": (_gemm_args(128, 320, 32, [(64, 9, True, 32)], w_layout=3, tile=64320, stat_part=_P, stat_cpg=10), False),
    "resid_rows": (_gemm_args(128, 320, 64, [(64, 1, False, 0)], w_layout=3, tile=64320, resid=_P, resid_ld=320, resid_rows=_P), False),
    "row LayerNorm": (_gemm_args(_M, 320, 256, [(320, 1, False, 0)], w_layout=3, tile=64320, ln_gamma=_P, ln_beta=_P, out_pl_ld=320,
                                 **_PLANES), False),
    "a32 source": (_gemm_args(_M, 320, 256, [(320, 1, False, 256)], w_layout=3, a32=_P, a32_ld=320, a32_part=_P, a32_nchunk=4, a32_pcpg=10,
                              a32_cpg=10, a32_gamma=_P, a32_beta=_P), False),
    "GroupNorm of the result, 64 x 80": (_gemm_args(64 * 64, 640, 64, [(640, 9, True, 64)], w_layout=3, tile=64080, slab_rows=16, stat_part=_P,
                                                    stat_cpg=20, gn_gamma=_P, gn_beta=_P, gn_cpg=20, out_pl_ld=640, **_PLANES), False),
    "128 x 160 tiles of the same kernel": (_gemm_args(_M, 320, 256, [(320, 9, True, 256)], w_layout=3, tile=128160, slab_rows=32), False),
    "the LDS-staged kernels": (_gemm_args(_M, 320, 256, [(320, 9, True, 256)], tile=128160), False),
    "a K cut": (_gemm_args(512, 320, 256, [(640, 9, True, 256)], w_layout=3, tile=64320, ksplit=4), False),
}


@pytest.mark.parametrize("name", sorted(_TABLE))
def test_resolved_bit_follows_the_predicate(name):
    a, want = _TABLE[name]
    lib = N.lib()
    a.dbg = ON
    on = _resolve(a)
    assert bool(on.dbg & ON) == want and not on.dbg & OFF, f"resolved dbg {on.dbg:#x}"
    if on.w_layout == 3 and on.tile in (64320, 64080):
        assert lib.wd_epilogue_batch_applies(ctypes.byref(on), 64, on.tile % 1000) == int(want)
        # the bit names the form of the 16-byte path; a call whose addresses keep it off that path runs the element loop either way
        if not a.stat_part:  # (statistics need the 16-byte path: wd_gemm_check refuses such a call)
            a.out_f32 = _P + 4
            odd = _resolve(a)
            assert bool(odd.dbg & ON) == want and lib.wd_epilogue_batch_applies(ctypes.byref(odd), 64, odd.tile % 1000) == 0
            a.out_f32 = _P
    a.dbg = OFF
    off = _resolve(a)
    assert not off.dbg & (ON | OFF)
    on.dbg &= ~ON
    assert bytes(on) == bytes(off)  # the switch decides nothing else


@pytest.mark.parametrize("switch", ["WD_GEMMW_SLAB", "WD_EPI_BATCH"])
def test_request_bits_resolve_on_the_smallest_slab_shape(switch):
    """The smallest legal slab launch (one 64 x 320 tile: a 3x3 source of 64 channels over one 8 x 8 image): *_ON resolves to
    *_BIT, *_OFF clears it, and neither request bit of the switch is left in the args wd_gemm_check returns.  ksplit = 1: neither
    form goes with a K cut, which wd_gemm would otherwise choose for a grid of one tile."""
    on_bit, off_bit, bit = (N.DEFINES[f"{switch}_{k}"] for k in ("ON", "OFF", "BIT"))
    a = _gemm_args(64, 320, 64, [(64, 9, True, 64)], w_layout=3, tile=64320, slab_rows=8, ksplit=1)
    a.dbg = on_bit
    assert _resolve(a).dbg & (on_bit | off_bit) == bit
    a.dbg = off_bit
    assert _resolve(a).dbg & (on_bit | off_bit | bit) == 0


def test_predicate_on_single_conditions():
    """wd_epilogue_batch_applies on one accepted set of resolved args, then each condition broken alone."""
    lib = N.lib()
    base = dict(w_layout=3, tile=64320, ksplit=1, bias=_P, rowvec=_P, rowvec_ld=320, resid=_P, resid_ld=324, out_pl_ld=328, stat_part=_P,
                stat_cpg=10, **_PLANES)

    def ok(bm=64, bn=320, m=128, hw_out=64, **kw):
        a = _gemm_args(m, 320, hw_out, [(64, 9, True, hw_out)], **dict(base, **kw))
        return lib.wd_epilogue_batch_applies(ctypes.byref(a), bm, bn)

    assert ok() == 1 and ok(act=N.ACT_SILU) == 1 and ok(bn=80) == 1 and ok(hw_out=128, m=256) == 1
    assert ok(act=N.ACT_GEGLU) == 0
    assert ok(ksplit=2) == 0
    assert ok(ln_gamma=_P) == 0 and ok(gn_gamma=_P) == 0 and ok(a32=_P) == 0
    assert ok(resid_rows=_P) == 0
    assert ok(m=96) == 0                      # last tile ragged in M
    assert ok(bn=160 + 80 + 160) == 0         # n = 320 is no multiple of 400 columns
    assert ok(hw_out=32) == 0 and ok(hw_out=96, m=192) == 0   # two samples per panel / a tile across two samples
    assert ok(resid_ld=322) == 0 and ok(out_f32=_P + 4) == 0 and ok(out_hi=_P + 2) == 0   # off the 16-byte path
    assert ok(out_ld=1 << 22) == 0            # a tile's byte offsets would not fit 31 bits
    assert ok(bm=128) == 0                    # the 128-row kernels keep the row loop
    assert lib.wd_epilogue_batch_applies(None, 64, 320) == 0


def _ff_args(m, hw_out, **fields):
    a = N.WdFfArgs()
    a.x_hi = a.x_lo = a.w1_hi = a.w1_lo = a.w2_hi = a.w2_lo = a.b1 = a.b2 = _P
    a.x_ld, a.m, a.c, a.inner, a.npass, a.hw_out = 320, m, 320, 1280, 3, hw_out
    a.resid, a.resid_ld, a.out_f32, a.out_ld = _P, 320, _P, 320
    for k, v in fields.items():
        setattr(a, k, v)
    return a


_PROJ = dict(w3_hi=_P, w3_lo=_P, b3=_P, resid3=_P, resid3_ld=320)
_FF = {
    "plain tail": (_ff_args(_M, 256), True),
    "proj_out with statistics": (_ff_args(_M, 256, stat_part=_P, stat_cpg=10, **_PROJ), True),
    "folded tail with statistics": (_ff_args(_M, 256, stat_part=_P, stat_cpg=10, w32_hi=_P, w32_lo=_P, b32=_P, **_PROJ), True),
    "ragged m": (_ff_args(130, 64), False),
    "hw_out = 1 (no sample grid given)": (_ff_args(_M, 1), False),
    "two samples per panel": (_ff_args(128, 32, stat_part=_P, stat_cpg=10, **_PROJ), False),
}


@pytest.mark.parametrize("name", sorted(_FF))
def test_wd_ff_check_resolves_the_bit(name):
    a, want = _FF[name]
    lib = N.lib()
    out = N.WdFfArgs()
    a.dbg = ON
    req = bytes(a)
    assert lib.wd_ff_check(ctypes.byref(a), ctypes.byref(out)) == N.WD_OK and bytes(a) == req
    assert bool(out.dbg & ON) == want and not out.dbg & OFF
    a.dbg = OFF
    assert lib.wd_ff_check(ctypes.byref(a), ctypes.byref(out)) == N.WD_OK and out.dbg == 0
    assert lib.wd_ff_check(ctypes.byref(a), None) == N.WD_OK and lib.wd_ff_check(None, None) == N.WD_EINVAL
    assert N.lib().wd_ff_args_bytes() == ctypes.sizeof(N.WdFfArgs)


def test_wd_ff_check_refuses_what_wd_ff_fused_refuses():
    a = _ff_args(_M, 256, out_ld=322)
    assert N.lib().wd_ff_check(ctypes.byref(a), None) == N.WD_EINVAL
    assert N.lib().wd_ff_fused(ctypes.byref(a), None) == N.WD_EINVAL  # (returns before any HIP call)

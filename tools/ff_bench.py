#!/usr/bin/env python3
"""Micro-benchmark of wd_ff_fused at the 8x32 level of the headline batch (run on the GPU box).

    python tools/ff_bench.py [--proj 1] [--iters 30]        WDIFF_LIB=<other .so> for A/B builds of the kernel
    python tools/ff_bench.py --front 1 [--m 16384 | --m 64]  the launch with the transformer front (GroupNorm + proj_in + both
                                                             cross-attentions + norm3 ahead of the feed-forward), random block of
                                                             tests/test_gpu_st_fused.py: the full chip (m = 16384: 256 panels) or
                                                             one workgroup alone (m = 64: one sample of 64 tokens)
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.engine import geglu_interleave  # noqa: E402

DEV = "cuda:0"


def planes(x):
    hi = x.to(torch.bfloat16)
    return torch.stack([hi, (x - hi.float()).to(torch.bfloat16)], 0).contiguous()


def timed(launch, iters):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def _epi_dbg(epi_batch):
    """wd_ff_args.dbg for --epi-batch: 1 / 0 = the batched epilogue where legal / the row loop, whatever WDIFF_EPI_BATCH says."""
    return 0 if epi_batch < 0 else N.EPI_BATCH_ON if epi_batch else N.EPI_BATCH_OFF


def front(m, iters, epi_batch=-1):
    from tests.test_gpu_st_fused import _Block  # the seeded transformer block the fused launch is tested on
    if m % 256 == 0:
        blk = _Block(m // 256)
    elif m == 64:  # one panel: the same block as one sample of 64 tokens
        blk = _Block(1)
        blk.hw = blk.m = 64
        blk.x = blk.x[:64].contiguous()
        blk.nchunk = blk.lib.wd_gn_nchunk(64)
        blk.part = torch.zeros(1, blk.nchunk, 32, 2, dtype=torch.float64, device=DEV)
        N.check(blk.lib.wd_gn_stats(blk.x.data_ptr(), blk.c, 1, 64, blk.c, blk.c // 32, blk.part.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "stats")
    else:
        sys.exit("--front: m is a multiple of 256 (samples of 8 x 32 tokens) or 64 (one workgroup)")
    out = torch.empty(blk.m, blk.c, device=DEV)
    stat = torch.empty(blk.B, blk.hw // 64, 32, 2, dtype=torch.float64, device=DEV)
    tok2 = torch.empty(blk.m, blk.c, device=DEV)
    f = blk.fused_args(out, stat, tok2)
    f.dbg = _epi_dbg(epi_batch)
    r = N.WdFfArgs()
    N.check(blk.lib.wd_ff_check(C.byref(f), C.byref(r)), "wd_ff_check")
    st = torch.cuda.current_stream().cuda_stream
    N.check(blk.lib.wd_ff_fused(C.byref(f), st), "wd_ff_fused (front)")
    us = timed(lambda: blk.lib.wd_ff_fused(C.byref(f), st), iters)
    print(f"wd_ff_fused front m={blk.m} ({blk.m // 64} workgroups) epi_batch={int(bool(r.dbg & N.EPI_BATCH_BIT))}: {us:7.1f} us   lib {N.LIB_PATH}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proj", type=int, default=1)
    ap.add_argument("--front", type=int, default=0)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--epi-batch", type=int, default=-1, help="1 / 0: the epilogue takes its batched form where legal / keeps the row loop "
                    "(wd_ff_args.dbg WD_EPI_BATCH_ON / _OFF), whatever WDIFF_EPI_BATCH says")
    a = ap.parse_args()
    if a.front:
        return front(a.m, a.iters, a.epi_batch)
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    m, c, inner = a.m, 320, 1280
    g = torch.Generator().manual_seed(0)
    x = torch.randn(m, c, generator=g).to(DEV)
    w1 = (torch.randn(2 * inner, c, generator=g) / c ** 0.5).to(DEV)
    w2 = (torch.randn(c, inner, generator=g) / inner ** 0.5).to(DEV)
    w3 = (torch.randn(c, c, generator=g) / c ** 0.5).to(DEV)
    b1, b2, b3 = torch.randn(2 * inner, device=DEV), torch.randn(c, device=DEV), torch.randn(c, device=DEV)
    res, res3 = torch.randn(m, c, device=DEV), torch.randn(m, c, device=DEV)

    def pack(w):
        wp = planes(w)
        wf = torch.empty_like(wp)
        N.check(lib.wd_gemm_pack_w(wp[0].data_ptr(), wp[1].data_ptr(), wp.shape[1], wp.shape[2], wf[0].data_ptr(), wf[1].data_ptr(), st), "pack")
        return wf

    w1f, w2f, w3f = pack(geglu_interleave(w1, 16)), pack(w2), pack(w3)
    b1i = geglu_interleave(b1, 16).contiguous()
    xp = planes(x)
    out = torch.empty(m, c, device=DEV)
    f = N.WdFfArgs()
    f.x_hi, f.x_lo, f.x_ld = xp[0].data_ptr(), xp[1].data_ptr(), c
    f.m, f.c, f.inner = m, c, inner
    f.w1_hi, f.w1_lo, f.b1 = w1f[0].data_ptr(), w1f[1].data_ptr(), b1i.data_ptr()
    f.w2_hi, f.w2_lo, f.b2 = w2f[0].data_ptr(), w2f[1].data_ptr(), b2.data_ptr()
    f.resid, f.resid_ld = res.data_ptr(), c
    f.out_f32, f.out_ld = out.data_ptr(), c
    if a.proj:
        f.w3_hi, f.w3_lo, f.b3 = w3f[0].data_ptr(), w3f[1].data_ptr(), b3.data_ptr()
        f.resid3, f.resid3_ld = res3.data_ptr(), c
    f.hw_out, f.npass = 1, 3
    f.dbg = _epi_dbg(a.epi_batch)
    N.check(lib.wd_ff_fused(C.byref(f), st), "wd_ff_fused")
    us = timed(lambda: lib.wd_ff_fused(C.byref(f), st), a.iters)
    fl = 2.0 * m * (3.0 * inner * c + (c * c if a.proj else 0))
    print(f"wd_ff_fused m={m} proj={a.proj}: {us:7.1f} us  {fl / us / 1e6:6.1f} TF/s algorithmic ({3 * fl / us / 1e6:6.1f} MFMA)   lib {N.LIB_PATH}")


if __name__ == "__main__":
    main()

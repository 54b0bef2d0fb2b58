"""Two kernels of the production sampling plan that only the end-to-end goldens reached: wd_select_rows (the first launch of every
step: the FiLM rows of the current timestep out of the resident table) and wd_gn_fold_chunks (GroupNorm chunk sums folded once per
sample), behind guard bands (tests/_guard.py).  (The third one, the raw planes of wd_xattn_planes: tests/test_gpu_xattn_guard.py.)

Seen on an MI355X: wd_select_rows bit-exact; gn_fold_chunks_kernel 2.5e-16 of the fp64 sum at most (max_rel; bound 1e-15);
wd_gn_apply on the folded / the raw statistics 4.5e-06 / 4.5e-06 of the fp64 GroupNorm (bound 3e-5), the same bits from both on
the two cases here."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tests import _guard as G  # noqa: E402
from tests._common import max_rel  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("row_floats", [4, 20, 4100])
def test_select_rows_behind_guard_bands(B, row_floats):
    """out[b] = table[(*t_dev) % chunk][b], bit for bit, for *t_dev below, at and beyond the chunk (the wrap the header documents:
    one resident chunk serves all timesteps), nothing written outside out, nothing read outside the table (its pads are NaN).

    A negative *t_dev cannot reach the kernel (C's % would keep the sign and the read start before the table): the index is
    P.t_dev or P.k_dev (engine.py _film_table); diffusion.py fills t_dev with the sampler's first timestep (>= 0) and steps it down by
    one after each step of the DDPM loop, whose last selecting step is t = 1; k_dev starts at zero and wd_next_timestep clamps it
    to [0, S - 1]."""
    lib = N.lib()
    chunk = 5
    g = torch.Generator().manual_seed(B + row_floats)
    tbuf, table = G.guarded_flat(chunk * B * row_floats, torch.float32, device=DEV)
    table.copy_(torch.randn(chunk * B * row_floats, generator=g))
    rows = table.view(chunk, B * row_floats).view(torch.int32).cpu()
    t_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    for t in (0, 1, chunk - 1, chunk, 2 * chunk + 3):
        t_dev.fill_(t)
        obuf, out = G.guarded_flat(B * row_floats, torch.float32, device=DEV)
        N.check(lib.wd_select_rows(table.data_ptr(), t_dev.data_ptr(), B, row_floats, chunk, out.data_ptr(), _st()), "wd_select_rows")
        torch.cuda.synchronize()
        G.assert_untouched(obuf, out, f"wd_select_rows out (t={t})")
        G.assert_untouched(tbuf, table, "wd_select_rows table")
        assert torch.equal(out.view(torch.int32).cpu(), rows[t % chunk]), f"t = {t}: not row {t % chunk} of the table"
    out = torch.zeros(B * row_floats + 8, device=DEV)
    assert lib.wd_select_rows(table.data_ptr(), t_dev.data_ptr(), B, 6, chunk, out.data_ptr(), _st()) == N.WD_EINVAL
    assert lib.wd_select_rows(table.data_ptr(), t_dev.data_ptr(), B, row_floats, 0, out.data_ptr(), _st()) == N.WD_EINVAL
    assert lib.wd_select_rows(table.data_ptr(), t_dev.data_ptr(), B, row_floats, -3, out.data_ptr(), _st()) == N.WD_EINVAL
    assert lib.wd_select_rows(table.data_ptr(), t_dev.data_ptr(), 0, row_floats, chunk, out.data_ptr(), _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ngroups", [1, 8, 32])
def test_gn_fold_chunks_behind_guard_bands(B, ngroups):
    """out[b][g] = sum over the chunks of part[b][:][g] in fp64 - within 1e-15 of torch's sum (the fixed order, four strided lanes
    and a pairwise finish, differs from it only in association), the same bits from a second launch, nothing written outside;
    nchunk 1 to 5 are the edges of the four-lane stride, 9 a third pass."""
    lib = N.lib()
    g = torch.Generator().manual_seed(10 * B + ngroups)
    worst = 0.0
    for nchunk in (1, 2, 3, 4, 5, 9):
        part = torch.randn(B, nchunk, ngroups, 2, generator=g, dtype=torch.float64) * 40.0
        part[..., 1] = part[..., 1] ** 2   # (sum, sum of squares)
        pbuf, pv = G.guarded_flat(part.numel(), torch.float64, device=DEV)
        pv.copy_(part.reshape(-1))
        outs = []
        for _ in range(2):
            obuf, out = G.guarded_flat(B * ngroups * 2, torch.float64, device=DEV)
            N.check(lib.wd_gn_fold_chunks(pv.data_ptr(), B, nchunk, ngroups, out.data_ptr(), _st()), "wd_gn_fold_chunks")
            torch.cuda.synchronize()
            G.assert_untouched(obuf, out, f"wd_gn_fold_chunks out (nchunk={nchunk})")
            G.assert_finite(out, "wd_gn_fold_chunks out")
            outs.append(out.cpu())
        G.assert_untouched(pbuf, pv, "wd_gn_fold_chunks part")
        assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
        ref = part.sum(1).reshape(-1)
        err = float(((outs[0] - ref).abs() / ref.abs().clamp_min(1e-300)).max()) if nchunk == 1 else max_rel(outs[0], ref)
        worst = max(worst, err)
        assert err <= 1e-15, f"nchunk = {nchunk}: {err:.3g}"
        if nchunk == 1:
            assert torch.equal(outs[0], ref)
    print(f"ERR gn_fold_chunks_kernel (B={B}, ngroups={ngroups}): {worst:.2e}")
    out = torch.zeros(B * 34 * 2, dtype=torch.float64, device=DEV)
    big = torch.ones(B * 2 * 33 * 2, dtype=torch.float64, device=DEV)
    assert lib.wd_gn_fold_chunks(big.data_ptr(), B, 2, 33, out.data_ptr(), _st()) == N.WD_EINVAL
    assert lib.wd_gn_fold_chunks(big.data_ptr(), B, 0, 8, out.data_ptr(), _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())


@pytest.mark.parametrize("c,cpg,hw", [(64, 2, 270), (320, 10, 130)])
def test_gn_apply_takes_the_folded_statistics(c, cpg, hw):
    """wd_gn_apply gives the same planes from the folded array with nchunk = 1 as from the raw one with the real nchunk, to 3e-5 -
    not bit for bit: wd_gn_apply adds a sample's chunks one after the other, wd_gn_fold_chunks adds four strided partial sums
    pairwise, and from four chunks on the two orders round differently in the last bit of the fp64 sums (which the fp32 mean and
    rstd mostly, not always, absorb)."""
    lib = N.lib()
    B, ng = 2, c // cpg
    g = torch.Generator().manual_seed(c + hw)
    x = torch.randn(B * hw, c, generator=g) * 2.0 + 0.5
    ga, be = torch.randn(c, generator=g) * 0.2 + 1.0, torch.randn(c, generator=g) * 0.2
    ref = F.group_norm(x.double().view(B, hw, c).permute(0, 2, 1), ng, ga.double(), be.double(), 1e-5).permute(0, 2, 1).reshape(B * hw, c)
    xd, gd, bd = x.to(DEV), ga.to(DEV), be.to(DEV)
    nchunk = lib.wd_gn_nchunk(hw)
    assert nchunk >= 5
    part = torch.zeros(B, nchunk, ng, 2, dtype=torch.float64, device=DEV)
    N.check(lib.wd_gn_stats(xd.data_ptr(), c, B, hw, c, cpg, part.data_ptr(), _st()), "wd_gn_stats")
    fbuf, folded = G.guarded_flat(B * ng * 2, torch.float64, device=DEV)
    N.check(lib.wd_gn_fold_chunks(part.data_ptr(), B, nchunk, ng, folded.data_ptr(), _st()), "wd_gn_fold_chunks")
    planes = []
    for p, nck in ((folded, 1), (part, nchunk)):
        pbuf, pl = G.guarded(B * hw, c, c + 8, 4, torch.bfloat16, device=DEV, planes=2)
        N.check(lib.wd_gn_apply(xd.data_ptr(), c, B, hw, c, cpg, p.data_ptr(), nck, cpg, gd.data_ptr(), bd.data_ptr(), 1e-5, 0,
                                pl[0].data_ptr(), pl[1].data_ptr(), c + 8, 0, None, None, _st()), "wd_gn_apply")
        torch.cuda.synchronize()
        G.assert_untouched(pbuf, pl, f"wd_gn_apply planes (nchunk={nck})")
        G.assert_finite(pl, "wd_gn_apply planes")
        planes.append((pl[0].float() + pl[1].float()).cpu())
    G.assert_untouched(fbuf, folded, "wd_gn_fold_chunks out")
    assert max_rel(folded.cpu().view(B, ng, 2), part.sum(1).cpu()) <= 1e-15
    e0, e1, e01 = max_rel(planes[0], ref), max_rel(planes[1], ref), max_rel(planes[0], planes[1])
    print(f"ERR wd_gn_apply folded / raw statistics (c={c}, hw={hw}): {e0:.2e} / {e1:.2e}, between them {e01:.2e}")
    assert e0 < 3e-5 and e1 < 3e-5 and e01 < 3e-5

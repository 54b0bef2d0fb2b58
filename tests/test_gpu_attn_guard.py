"""The forward attention family (csrc/wd_attn.hip: wd_attention and its three kernels, wd_attention_pack_kv, wd_attention_packed)
behind guard bands and on staircase logits.

Every operand is a window of a wider, taller buffer whose every other element is a NaN pattern (tests/_guard.py), laid out as the
engine passes them: q with ldq = inner + 8 at column 4; K and V two windows of ONE buffer (one pitch, K at column 4, V at column
inner + 12, NaN columns between and around them, NaN rows before the first sample and after the last); the outputs one window per
sample (out_rows = nq + 3, out_row0 = 2, column 4) of poisoned buffers.  wd_attention has ONE out_ld for the fp32 result and the
planes: inner + 12 where the fp32 result is written, inner + 8 for the planes alone.  Each case runs with fp32 + planes, planes
only (out_f32 = NULL) and without the lo plane (out_lo = NULL), and asserts: windows finite (a read outside an operand brings a
NaN in), fp32 within 2e-5 and planes within 3e-5 of fp64 (max_rel, the tolerances of tests/test_gpu_kernels.py), every element
outside the per-sample windows still the poison bits, the same bits in every run and in a dense launch (all pitches = the width).

The staircase cases (tests/_attn_ref.py; gated on the host by tests/test_attn_ref_host.py) run the online softmax of
attn_mfma_kernel with a live accumulator: the maximum moves by 7 nats (10.1 log2 units > FA_LAZY) at every stair, or by 3 / 4 nats
(exponentials up to 2^7, a rescale every third / second stair), the two key groups of the 64-query form end on different maxima.

Largest max_rel against fp64 seen on an MI355X (fp32 result / planes; tolerances 2e-5 / 3e-5), and the cases that reach each kernel:
  attn_small_kernel<10>        SMALL rows with nk = 10, the small staircase with nk = 10          2.2e-07 / 5.8e-06
  attn_small_kernel<0>         SMALL rows with nk in {1, 7, 16}, the small staircase with nk = 16  2.3e-07 / 5.7e-06
  attn_kernel                  GENERIC rows, the forced MFMA shapes, the generic staircase         6.9e-06 / 9.0e-06
  attn_mfma_kernel<KS, KSPLIT> MFMA rows with nq <= 64, staircase cases with nq <= 64, per KS = 1..6:
                               7.9e-06 / 8.9e-06, 7.3e-06 / 9.3e-06, 5.4e-06 / 7.1e-06, 6.3e-06 / 9.5e-06, 6.9e-06 / 6.7e-06, 9.3e-06 / 1.1e-05
  attn_mfma_kernel<KS>         MFMA rows with nq > 64, staircase cases with nq > 64, per KS = 1..6:
                               8.5e-06 / 1.0e-05, 6.1e-06 / 8.0e-06, 7.2e-06 / 9.0e-06, 1.0e-05 / 1.0e-05, 9.6e-06 / 9.9e-06, 5.8e-06 / 7.1e-06
  ... PACKED                   the packed rows (KS = 2 and 5, both forms) and every staircase case: the bits of the unpacked launch
                               (asserted), 6.5e-06 / 7.8e-06 at most on the packed rows
  attn_pack_kernel             the packed rows (<2, 1> and <5, 3>): every image element written, repeatable bits
The largest figures are the staircase cases (1.0e-05 on the 3-nat stairs over 300 keys, d = 64)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _attn_ref as R  # noqa: E402
from tests import _guard as G  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

DEV = "cuda:0"
TOL_F32, TOL_PL = 2e-5, 3e-5
NKS = 16  # csrc/wd_attn.hip


def _st():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def kernel_of(H, nq, nk, d, out_ld, generic=False):
    """The dispatch rule of wd_attention (csrc/wd_attn.hip), for the record each case prints."""
    inner, tpw = H * d, 256 // H
    small_smem = (2 * nk * inner + tpw * (inner + 4)) * 4
    if nk <= NKS and H <= 256 and small_smem <= 150 * 1024 and out_ld % 4 == 0 and not generic:
        return "attn_small_kernel<10>" if nk == 10 else "attn_small_kernel<0>"
    if nk > NKS and d % 16 == 0 and d <= 96 and out_ld % 4 == 0 and not generic:
        return f"attn_mfma_kernel<KS={d // 16}{', KSPLIT' if nq <= 64 else ''}>"
    return "attn_kernel"


@functools.lru_cache(maxsize=None)
def _plain(B, H, nq, nk, d, scale):
    """(q, k, v, fp64 reference) of a 0.5 * randn case, computed once and shared (never modified)."""
    g = torch.Generator().manual_seed(7 * nq + 3 * nk + d + H)
    q, k, v = (torch.randn(B * n, H * d, generator=g) * 0.5 for n in (nq, nk, nk))
    return q, k, v, R.attention_fp64(q, k, v, B, H, nq, nk, d, scale)


@functools.lru_cache(maxsize=None)
def _stairs(B, H, nq, nk, d, scale, step, period, desc):
    q, k, v, _ = R.staircase(B, H, nq, nk, d, scale, step, period, desc)
    return q, k, v, R.attention_fp64(q, k, v, B, H, nq, nk, d, scale)


def _kv_buffer(k, v, B, nk, inner, dense):
    """K and V as the engine holds them: two windows of one pitched buffer.  Returns (buffer, k pointer, v pointer, pitch)."""
    if dense:
        kd, vd = k.to(DEV).contiguous(), v.to(DEV).contiguous()
        return (kd, vd), kd.data_ptr(), vd.data_ptr(), inner
    ld = 2 * inner + 16
    buf = G.poisoned((B * nk + 4, ld), torch.float32)
    buf[2:2 + B * nk, 4:4 + inner] = k
    buf[2:2 + B * nk, inner + 12:2 * inner + 12] = v
    buf = buf.to(DEV)
    return buf, buf[2, 4:].data_ptr(), buf[2, inner + 12:].data_ptr(), ld


def _outputs(B, nq, inner, out_ld, dense, dtype, planes=0):
    """(buffer, pointer(s), windows, gather): the per-sample output windows inside a poisoned buffer."""
    lead = (planes,) if planes else ()
    if dense:
        buf = G.poisoned(lead + (B * nq, inner), dtype, DEV)
        return buf, buf, [(0, B * nq, 0, inner)], lambda t: t
    out_rows, g, col0 = nq + 3, 2, min(4, out_ld - inner)  # (out_ld = inner + 2: the window ends with the row)
    buf = G.poisoned(lead + (2 * g + B * out_rows, out_ld), dtype, DEV)
    wins = G.row_windows(B, out_rows, g + 2, nq, col0, inner)
    view = buf[..., g:, col0:]  # the address wd_attention gets: row 0 of sample 0's out_rows, column 0 of the window

    def gather(t):
        return torch.cat([t[..., r0:r0 + nq, col0:col0 + inner] for r0, _, _, _ in wins], -2)
    return buf, view, wins, gather


def launch(q, k, v, B, H, nq, nk, d, scale, mode="both", dense=False, extra=None, img=None):
    """One wd_attention (img: wd_attention_packed) launch.  mode: 'both' fp32 + planes, 'planes' out_f32 = NULL, 'nolo' out_lo =
    NULL.  extra: columns beyond inner of out_ld (default 12 with the fp32 result, 8 without).  Returns (fp32 window or None,
    planes window [2][B * nq][inner] with the lo plane absent in 'nolo'), both on the host; asserts that nothing outside the
    windows changed."""
    lib = N.lib()
    inner = H * d
    extra = (8 if mode == "planes" else 12) if extra is None else extra
    out_ld = inner if dense else inner + extra
    qbuf, qv = (None, q.to(DEV).contiguous()) if dense else G.pitched(q, inner + 8, 4, device=DEV)
    ldq = inner if dense else inner + 8
    kvbuf, kp, vp, ldkv = _kv_buffer(k, v, B, nk, inner, dense)
    fbuf, fview, wins, gather = _outputs(B, nq, inner, out_ld, dense, torch.float32)
    pbuf, pview, _, _ = _outputs(B, nq, inner, out_ld, dense, torch.bfloat16, planes=2)
    f_ptr = None if mode == "planes" else fview.data_ptr()
    hi_ptr, lo_ptr = pview[0].data_ptr(), None if mode == "nolo" else pview[1].data_ptr()
    tail = (f_ptr, hi_ptr, lo_ptr, out_ld, nq if dense else nq + 3, 0 if dense else 2, _st())
    if img is None:
        N.check(lib.wd_attention(qv.data_ptr(), ldq, kp, ldkv, vp, ldkv, B, H, nq, nk, d, scale, *tail), "wd_attention")
    else:
        N.check(lib.wd_attention_packed(qv.data_ptr(), ldq, img.data_ptr(), B, H, nq, nk, d, scale, *tail), "wd_attention_packed")
    torch.cuda.synchronize()
    what = f"(B={B}, H={H}, nq={nq}, nk={nk}, d={d}, {mode}{', dense' if dense else ''})"
    G.assert_untouched_windows(fbuf, [] if mode == "planes" else wins, "out_f32 " + what)
    G.assert_untouched_windows(pbuf[0], wins, "out_hi " + what)
    G.assert_untouched_windows(pbuf[1], [] if mode == "nolo" else wins, "out_lo " + what)
    if qbuf is not None:
        G.assert_untouched(qbuf, qv, "q " + what)
    f = None if mode == "planes" else gather(fbuf).cpu()
    p = gather(pbuf).cpu()
    if f is not None:
        G.assert_finite(f, "out_f32 " + what)
    G.assert_finite(p[:1] if mode == "nolo" else p, "planes " + what)
    return f, (p[:1] if mode == "nolo" else p)


def check_case(q, k, v, ref, B, H, nq, nk, d, scale, generic=False, extra=None, dense_bits=True, img=None):
    """The three runs of one case + the dense launch; returns (kernel, fp32 error, planes error)."""
    inner = H * d
    kern = kernel_of(H, nq, nk, d, inner + (12 if extra is None else extra), generic)
    f, p = launch(q, k, v, B, H, nq, nk, d, scale, "both", extra=extra, img=img)
    ef, ep = R.max_rel(f, ref), R.max_rel(p[0].float() + p[1].float(), ref)
    print(f"ERR {kern}{' PACKED' if img is not None else ''} (B={B}, H={H}, nq={nq}, nk={nk}, d={d}): fp32 {ef:.2e} planes {ep:.2e}")
    assert ef < TOL_F32 and ep < TOL_PL
    assert torch.equal(p, G.split_planes(f))  # the planes are the split of the fp32 result
    if extra is None:  # (an out_ld the planes-only pitch would send to another kernel keeps its own pitch)
        _, p2 = launch(q, k, v, B, H, nq, nk, d, scale, "planes", img=img)
        assert torch.equal(p2, p)
    f3, p3 = launch(q, k, v, B, H, nq, nk, d, scale, "nolo", extra=extra, img=img)
    assert torch.equal(f3, f) and torch.equal(p3[0], p[0])
    if dense_bits:
        assert kernel_of(H, nq, nk, d, inner, generic) == kern
        fd, pd = launch(q, k, v, B, H, nq, nk, d, scale, "both", dense=True, img=img)
        assert torch.equal(fd, f) and torch.equal(pd, p)
    return kern, ef, ep


# ---- (H, nq, nk, d), B = 2.  attn_mfma_kernel<KS = d / 16>: nq <= 64 the key-split form (KSPLIT), nq > 64 the 128-query form
MFMA = [
    (1, 1, 17, 16),     # attn_mfma_kernel<1, KSPLIT>: one query, the first key count above NKS, the odd key group idle
    (2, 31, 32, 32),    # attn_mfma_kernel<2, KSPLIT>: exactly one sub-block, the odd key group idle
    (3, 33, 33, 48),    # attn_mfma_kernel<3, KSPLIT>: one key past a sub-block - the odd group holds a single key
    (1, 64, 63, 64),    # attn_mfma_kernel<4, KSPLIT>: a partial block, a full query tile
    (2, 1, 64, 80),     # attn_mfma_kernel<5, KSPLIT>: exactly one block
    (3, 31, 65, 96),    # attn_mfma_kernel<6, KSPLIT>: a block and one key - the even group gets it
    (1, 33, 96, 16),    # attn_mfma_kernel<1, KSPLIT>: a block and a sub-block - the odd group one sub-block short
    (2, 64, 129, 32),   # attn_mfma_kernel<2, KSPLIT>
    (3, 64, 200, 48),   # attn_mfma_kernel<3, KSPLIT>
    (2, 33, 17, 64),    # attn_mfma_kernel<4, KSPLIT>
    (1, 31, 96, 80),    # attn_mfma_kernel<5, KSPLIT>
    (2, 64, 33, 96),    # attn_mfma_kernel<6, KSPLIT>
    (1, 65, 17, 16),    # attn_mfma_kernel<1>: the first query count of the 128-query form
    (2, 127, 32, 32),   # attn_mfma_kernel<2>
    (3, 128, 33, 48),   # attn_mfma_kernel<3>: a full tile
    (1, 129, 63, 64),   # attn_mfma_kernel<4>: one query in the second tile
    (2, 257, 64, 80),   # attn_mfma_kernel<5>: three tiles
    (3, 65, 65, 96),    # attn_mfma_kernel<6>
    (1, 127, 96, 16),   # attn_mfma_kernel<1>
    (2, 128, 129, 32),  # attn_mfma_kernel<2>
    (3, 129, 200, 48),  # attn_mfma_kernel<3>
    (2, 257, 17, 64),   # attn_mfma_kernel<4>
    (1, 65, 96, 80),    # attn_mfma_kernel<5>
    (2, 129, 33, 96),   # attn_mfma_kernel<6>
]


@pytest.mark.parametrize("H,nq,nk,d", MFMA)
def test_mfma_attention_behind_guard_bands(H, nq, nk, d):
    B, scale = 2, d ** -0.5
    q, k, v, ref = _plain(B, H, nq, nk, d, scale)
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale)
    assert kern == f"attn_mfma_kernel<KS={d // 16}{', KSPLIT' if nq <= 64 else ''}>"


# ---- attn_kernel.  (H, nq, nk, d, extra columns of out_ld or None)
GENERIC = [
    (2, 13, 40, 20, None),    # attn_kernel: d % 16 != 0, nq % 8 != 0, nk > 16
    (2, 9, 300, 36, None),    # attn_kernel: nk > 256 - the second pass of its j += 256 loop
    (2, 8, 33, 128, None),    # attn_kernel: d > 96
    (1, 5, 40, 320, None),    # attn_kernel: one head of width 320 (Word_Attention's shape with more keys)
    (8, 32, 16, 80, None),    # attn_kernel: nk <= 16 but the small kernel would need 164 KB of LDS (> 150 KB)
    (2, 40, 65, 32, 2),       # attn_kernel: an attn_mfma_kernel<2, KSPLIT> shape with out_ld = inner + 2: fp32 rows off the 16-byte grid
    (2, 100, 33, 48, 2),      # attn_kernel: an attn_mfma_kernel<3> shape, the same
    (4, 70, 10, 80, 2),       # attn_kernel: the attn_small_kernel<10> shape, the same
]


@pytest.mark.parametrize("H,nq,nk,d,extra", GENERIC)
def test_generic_attention_behind_guard_bands(H, nq, nk, d, extra):
    B, scale = 2, d ** -0.5
    q, k, v, ref = _plain(B, H, nq, nk, d, scale)
    # (out_ld = inner + 2: the dense launch, out_ld = inner, is another kernel's - no common bits to compare)
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale, extra=extra, dense_bits=extra is None)
    assert kern == "attn_kernel"


@pytest.mark.parametrize("H,nq,nk,d", [(2, 70, 96, 80), (2, 33, 129, 16)])  # attn_mfma_kernel<5> / <1, KSPLIT> shapes -> attn_kernel
def test_mfma_shapes_forced_through_the_generic_kernel(H, nq, nk, d, monkeypatch):
    """WDIFF_ATTN_GENERIC is read at every call: the same operands through attn_kernel agree with the MFMA launch to 2e-5."""
    B, scale = 2, d ** -0.5
    q, k, v, ref = _plain(B, H, nq, nk, d, scale)
    fm, _ = launch(q, k, v, B, H, nq, nk, d, scale)
    monkeypatch.setenv("WDIFF_ATTN_GENERIC", "1")
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale, generic=True)
    fg, _ = launch(q, k, v, B, H, nq, nk, d, scale)
    monkeypatch.delenv("WDIFF_ATTN_GENERIC")
    assert kern == "attn_kernel" and not torch.equal(fg, fm) and R.max_rel(fg, fm) < TOL_F32


# ---- attn_small_kernel<10> (nk = 10) / <0>: tokens per workgroup tpw = 256 / heads
SMALL = [
    (4, 70, 10, 80),    # attn_small_kernel<10>: the production shape; 108 KB of LDS - the path that raises the dynamic limit
    (3, 85, 1, 16),     # attn_small_kernel<0>: a softmax of one key; 3 heads: tpw = 85, thread 255 has no token; one full workgroup
    (3, 86, 7, 4),      # attn_small_kernel<0>: one token in the second workgroup; d = 4
    (3, 171, 16, 16),   # attn_small_kernel<0>: nk = NKS; two full workgroups and one token
    (3, 86, 10, 16),    # attn_small_kernel<10>: the unrolled form with a head count that does not divide 256
    (1, 300, 16, 4),    # attn_small_kernel<0>: one head, tpw = 256
    (8, 33, 7, 16),     # attn_small_kernel<0>: tpw = 32, one token in the second workgroup
    (4, 64, 1, 80),     # attn_small_kernel<0>: nk = 1 at the production width, exactly one workgroup
    (1, 257, 10, 80),   # attn_small_kernel<10>: one head
]


@pytest.mark.parametrize("H,nq,nk,d", SMALL)
def test_small_attention_behind_guard_bands(H, nq, nk, d):
    B, scale = 2, d ** -0.5
    q, k, v, ref = _plain(B, H, nq, nk, d, scale)
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale)
    assert kern == ("attn_small_kernel<10>" if nk == 10 else "attn_small_kernel<0>")


# ---- staircase logits
@pytest.mark.parametrize("cs", R.STAIRCASE, ids=lambda cs: f"nq{cs[2]}-nk{cs[3]}-d{cs[4]}-step{cs[6]}-p{cs[7]}{'-desc' if cs[8] else ''}")
def test_mfma_attention_on_staircase_logits(cs):
    """The rescale of the running state with a live accumulator (o *= alpha, lsum *= alpha, 0 < alpha < 1), exponentials above 1
    inside the lazy headroom, the merge of two key groups with different maxima - and the packed form on the same operands."""
    B, H, nq, nk, d, scale, step, period, desc = cs
    q, k, v, ref = _stairs(*cs)
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale)
    assert kern.startswith("attn_mfma_kernel")
    f, _ = launch(q, k, v, B, H, nq, nk, d, scale)
    img = _pack(k, v, B, H, nk, d)[1]
    fp, _ = launch(q, k, v, B, H, nq, nk, d, scale, img=img)
    assert torch.equal(fp, f)


@pytest.mark.parametrize("cs", R.GENERIC_STAIRCASE, ids=lambda cs: f"nq{cs[2]}-nk{cs[3]}-d{cs[4]}-step{cs[6]}-p{cs[7]}{'-desc' if cs[8] else ''}")
def test_generic_attention_on_staircase_logits(cs, monkeypatch):
    B, H, nq, nk, d, scale, step, period, desc = cs
    q, k, v, ref = _stairs(*cs)
    monkeypatch.setenv("WDIFF_ATTN_GENERIC", "1")
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale, generic=True)
    monkeypatch.delenv("WDIFF_ATTN_GENERIC")
    assert kern == "attn_kernel"


@pytest.mark.parametrize("cs", R.SMALL_STAIRCASE, ids=lambda cs: f"nq{cs[2]}-nk{cs[3]}-d{cs[4]}{'-desc' if cs[6] else ''}")
def test_small_attention_on_staircase_logits(cs):
    """A 7-nat stair at every key: logits spanning 63 (nk = 10) and 105 (nk = 16) nats."""
    B, H, nq, nk, d, scale, desc = cs
    q, k, v, ref = _stairs(B, H, nq, nk, d, scale, 7, 1, desc)
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale)
    assert kern.startswith("attn_small_kernel")


# ---- wd_attention_pack_kv / wd_attention_packed
def _pack(k, v, B, H, nk, d, kv_edit=None):
    """(guard buffer, image window) of wd_attention_pack_kv on the pitched K / V buffer.  kv_edit(buffer rows): changes the K / V
    buffer (host side, [rows][pitch]) before the launch."""
    lib = N.lib()
    inner = H * d
    n = lib.wd_attention_packed_elems(B, H, nk, d)
    assert n > 0 and n % 8 == 0
    ld = 2 * inner + 16
    host = G.poisoned((B * nk + 4, ld), torch.float32)
    host[2:2 + B * nk, 4:4 + inner] = k
    host[2:2 + B * nk, inner + 12:2 * inner + 12] = v
    if kv_edit is not None:
        kv_edit(host)
    kv = host.to(DEV)
    ibuf, img = G.guarded_flat(n, torch.bfloat16, device=DEV)
    assert img.data_ptr() % 16 == 0
    N.check(lib.wd_attention_pack_kv(kv[2, 4:].data_ptr(), ld, kv[2, inner + 12:].data_ptr(), ld, B, H, nk, d, img.data_ptr(), _st()),
            "wd_attention_pack_kv")
    torch.cuda.synchronize()
    G.assert_untouched(ibuf, img, f"image (B={B}, H={H}, nk={nk}, d={d})")
    return ibuf, img


@pytest.mark.parametrize("H,nq,nk,d", [(2, 40, 65, 32),     # attn_pack_kernel<2, 1>, attn_mfma_kernel<2, KSPLIT, PACKED>
                                       (2, 100, 779, 32),   # attn_pack_kernel<2, 1>, attn_mfma_kernel<2, PACKED>: the product's context
                                       (2, 64, 779, 80),    # attn_pack_kernel<5, 3>, attn_mfma_kernel<5, KSPLIT, PACKED>
                                       (2, 129, 65, 80)])   # attn_pack_kernel<5, 3>, attn_mfma_kernel<5, PACKED>
def test_packed_keys_and_values_behind_guard_bands(H, nq, nk, d):
    B, scale = 2, d ** -0.5
    inner = H * d
    q, k, v, ref = _plain(B, H, nq, nk, d, scale)
    _, img = _pack(k, v, B, H, nk, d)
    bits = img.view(torch.int16).cpu()
    assert not bool((bits == G.NAN16).any()), "an image element was not written"
    G.assert_finite(img, "image")
    assert torch.equal(_pack(k, v, B, H, nk, d)[1].view(torch.int16).cpu(), bits)  # a second poisoned buffer: the same bits
    # sample b's image depends on sample b's nk keys alone: other values in the guard rows and in the other sample's rows
    per = bits.numel() // B
    for b in range(B):
        def edit(host, b=b):
            host[:2] = 3.0
            host[-2:] = -5.0
            o = 1 - b
            host[2 + o * nk:2 + (o + 1) * nk, 4:4 + inner] += 1.0
            host[2 + o * nk:2 + (o + 1) * nk, inner + 12:2 * inner + 12] -= 1.0
        other = _pack(k, v, B, H, nk, d, edit)[1].view(torch.int16).cpu()
        assert torch.equal(other[b * per:(b + 1) * per], bits[b * per:(b + 1) * per])
        assert not torch.equal(other[(1 - b) * per:(2 - b) * per], bits[(1 - b) * per:(2 - b) * per])
    kern, _, _ = check_case(q, k, v, ref, B, H, nq, nk, d, scale, img=img)
    f, p = launch(q, k, v, B, H, nq, nk, d, scale)
    fp, pp = launch(q, k, v, B, H, nq, nk, d, scale, img=img)
    assert torch.equal(fp, f) and torch.equal(pp, p)  # the bits of wd_attention on the same pitched K / V


def test_attention_entry_points_refuse_what_they_cannot_run():
    """Refused before any launch (WD_EINVAL): a q pitch that breaks the 16-byte rows, d % 4, a misaligned image, nk <= 16 packed."""
    lib = N.lib()
    B, H, nq, nk, d = 2, 2, 8, 40, 16
    inner = H * d
    q = torch.zeros(B * nq + 1, inner + 8, device=DEV)
    kv = torch.zeros(B * nk, 2 * inner, device=DEV)
    out = torch.zeros(B * nq, inner, device=DEV)
    img = torch.zeros(lib.wd_attention_packed_elems(B, H, nk, d) + 8, dtype=torch.bfloat16, device=DEV)
    qp, kp, vp, op, ip = q.data_ptr(), kv.data_ptr(), kv.data_ptr() + 4 * inner, out.data_ptr(), img.data_ptr()
    ok = (B, H, nq, nk, d, 0.25, op, None, None, inner, nq, 0, _st())
    assert lib.wd_attention(qp, inner + 2, kp, 2 * inner, vp, 2 * inner, *ok) == N.WD_EINVAL
    assert lib.wd_attention(qp, inner, kp, 2 * inner + 2, vp, 2 * inner, *ok) == N.WD_EINVAL
    assert lib.wd_attention(qp, inner, kp, 2 * inner, vp, 2 * inner, B, H, nq, nk, 6, 0.25, op, None, None, inner, nq, 0,
                            _st()) == N.WD_EINVAL
    assert lib.wd_attention(qp, inner, kp, 2 * inner, vp, 2 * inner, B, H, nq, nk, d, 0.25, None, None, None, inner, nq, 0,
                            _st()) == N.WD_EINVAL
    assert lib.wd_attention_packed_elems(B, H, 16, d) == 0 and lib.wd_attention_packed_elems(B, H, nk, 20) == 0
    assert lib.wd_attention_pack_kv(kp, 2 * inner, vp, 2 * inner, B, H, nk, d, ip + 2, _st()) == N.WD_EINVAL
    assert lib.wd_attention_pack_kv(kp, 2 * inner + 2, vp, 2 * inner, B, H, nk, d, ip, _st()) == N.WD_EINVAL
    assert lib.wd_attention_pack_kv(kp, 2 * inner, vp, 2 * inner, B, H, 16, d, ip, _st()) == N.WD_EINVAL
    pk = (B, H, nq, nk, d, 0.25, op, None, None, inner, nq, 0, _st())
    assert lib.wd_attention_packed(qp, inner, ip + 2, *pk) == N.WD_EINVAL
    assert lib.wd_attention_packed(qp, inner + 2, ip, *pk) == N.WD_EINVAL
    assert lib.wd_attention_packed(qp, inner, ip, B, H, nq, 16, d, 0.25, op, None, None, inner, nq, 0, _st()) == N.WD_EINVAL
    assert lib.wd_attention_packed(qp, inner, ip, B, H, nq, nk, d, 0.25, op, None, None, inner + 2, nq, 0, _st()) == N.WD_EINVAL
    torch.cuda.synchronize()
    assert not bool(out.any())  # nothing ran

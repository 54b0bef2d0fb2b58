"""Host specification of the weight-gradient kernel (wd_dw / wd_dw_group), written from the formula in include/wdiff_hip.h:

    grad[n][ci * ntaps + t] = sum over mm < m of  d[mm][n] * x[src(mm, t)][ci]

src(mm, t) = row mm (no table), or (mm // hw_out) * hw_src + gather[t][mm % hw_out] with a zero row where the entry is -1.  Plain fp64
torch, one matrix product per tap.  Beside the sum it returns S[n][ci * ntaps + t] = sum |d| * |x|, the scale of the element-wise
error bound (dw_beta) the GPU tests use.

Two deliberately WRONG variants show that the bound can tell a wrong kernel from a right one (tests/test_dw_ref_host.py):
"pad_row0" lets a padding tap read source row 0 of the sample instead of zeros, "short" leaves the last 32 tokens out.

CONV_CASES / LINEAR_CASES and the input generators are shared by tests/test_gpu_dw_guard.py and the host gate, so that the gate
speaks about the very inputs the GPU test uses."""
import numpy as np
import torch

from tests._guard import split_planes
from worddiffusion_amd.engine import conv_gather_table

VARIANTS = ("pad_row0", "short")


def dw_ref(d, x, ntaps=1, gather=None, hw_out=0, hw_src=0, variant=None):
    """d [m][n], x [rows][c] -> (grad, S), both fp64 [n][c * ntaps].  gather: int [ntaps][hw_out] (tensor or array) or None."""
    assert variant in (None,) + VARIANTS
    d, x = d.double(), x.double()
    m, n = d.shape
    c = x.shape[1]
    if variant == "short":
        d = d.clone()
        d[m - 32:] = 0.0
    mm = torch.arange(m)
    if gather is None:
        assert ntaps == 1
    else:
        gather = torch.as_tensor(np.asarray(gather), dtype=torch.int64).reshape(ntaps, hw_out)
    grad = torch.zeros(n, c, ntaps, dtype=torch.float64)
    S = torch.zeros(n, c, ntaps, dtype=torch.float64)
    for t in range(ntaps):
        if gather is None:
            rows = x[mm]
        else:
            e = gather[t][mm % hw_out]
            rows = x[(mm // hw_out) * hw_src + e.clamp_min(0)]
            if variant != "pad_row0":
                rows = rows * (e >= 0)[:, None].double()
        grad[:, :, t] = d.t() @ rows
        S[:, :, t] = d.abs().t() @ rows.abs()
    return grad.reshape(n, c * ntaps), S.reshape(n, c * ntaps)


def dw_beta(m, nslice):
    """|got - ref| <= dw_beta * S, element by element, ref on the plane-rounded operands.  2^-18: the lo.lo term the three-pass
    product drops, two roundings of 2^-9 each (bf16 keeps 8 significant bits).  The rest: one fp32 rounding (2^-24) per accumulated
    product - 3 m of them, three passes over m tokens - and per slice add, doubled for an accumulator that truncates."""
    return 2.0 ** -18 + 2.0 * (3 * m + nslice) * 2.0 ** -24


def rounded(x, npass=3):
    """What the kernel sees of the fp32 matrix x: hi + lo of the split-bf16 planes (npass 3) or hi alone (npass 1), fp64."""
    p = split_planes(x.float()).double()
    return p[0] + p[1] if npass == 3 else p[0]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 4321)


def linear_inputs(m, n, c, key=0):
    """(d [m][n], x [m][c]) fp32."""
    g = _gen(m, n, c, key)
    return torch.randn(m, n, generator=g), torch.randn(m, c, generator=g)


_MODES = {"same": 1, "down": 2, "up": 3}


def conv_inputs(mode, B, h, w, n, c, key=0):
    """(d [B * ho * wo][n], x [B * h * w][c], table int32 [9][ho * wo], hw_out, hw_src) of a 3x3 layer on an h x w INPUT map."""
    tab, ho, wo = conv_gather_table(h, w, mode)
    g = _gen(_MODES[mode], B, h, w, n, c, key)
    return torch.randn(B * ho * wo, n, generator=g), torch.randn(B * h * w, c, generator=g), tab, ho * wo, h * w


# the grouped launches: the 4x16 map at batch 2 (m = 128, hw_out = hw_src = 64); item i of a nine-tap group is
# conv_inputs(*GROUP_MAP, n, n, key=i), of a single-tap group linear_inputs(128, n, n, key=i)
GROUP_MAP = ("same", 2, 4, 16)
# (ntaps, nitems, n = c, nslice, npass)
GROUP_CASES = [(1, 1, 160, 2, 3), (1, 3, 160, 2, 3), (1, 3, 160, 1, 1), (9, 2, 160, 2, 3), (9, 3, 160, 1, 3), (9, 3, 320, 2, 3), (9, 2, 320, 1, 1)]

# id: (m, n, c, nslice, grad_ld - c, grad column, accumulate, npass)
LINEAR_CASES = {
    "m64_one_pass_of_each_loop": (64, 160, 160, 1, 12, 0, 0, 3),
    "m64_scalar_stores_accumulate": (64, 160, 160, 1, 13, 3, 1, 3),
    "m192_slices_of_1_and_2_units": (192, 160, 160, 2, 12, 4, 0, 3),
    "m192_three_workgroups": (192, 160, 160, 3, 13, 3, 0, 3),
    "m192_one_plane": (192, 160, 160, 2, 12, 0, 1, 1),
    "m192_two_column_tiles": (192, 160, 320, 2, 13, 3, 1, 3),
    "m320_ten_workgroups": (320, 320, 160, 5, 12, 4, 1, 3),
    "m320_4_slices_of_5_units": (320, 320, 160, 4, 13, 3, 0, 3),
    "m320_3_slices_of_5_units_one_plane": (320, 160, 160, 3, 12, 0, 0, 1),
    "m512_automatic_slices": (512, 160, 160, 0, 12, 4, 0, 3),
}

# id: (mode, B, h, w, n, c, nslice, grad_ld - 9 c, grad column, accumulate, npass); (h, w) is the layer's INPUT map
CONV_CASES = {
    "same8x8_c160_s1": ("same", 3, 8, 8, 160, 160, 1, 5, 3, 0, 3),
    "same8x8_c160_s2": ("same", 3, 8, 8, 320, 160, 2, 0, 0, 1, 3),
    "same8x8_c160_s3": ("same", 3, 8, 8, 160, 160, 3, 5, 3, 1, 3),
    "same8x8_c320_s1": ("same", 3, 8, 8, 160, 320, 1, 8, 4, 1, 3),
    "same8x8_c320_s2": ("same", 3, 8, 8, 160, 320, 2, 5, 3, 0, 1),
    "same8x8_c320_s3": ("same", 3, 8, 8, 320, 320, 3, 5, 3, 0, 3),
    "same8x16_slices_begin_inside_a_sample": ("same", 3, 8, 16, 160, 160, 4, 5, 3, 0, 3),
    "down16x16_to_8x8": ("down", 2, 16, 16, 160, 160, 2, 5, 3, 1, 3),
    "up4x8_to_8x16": ("up", 2, 4, 8, 160, 160, 2, 8, 4, 0, 3),
    "same32x32_largest_map": ("same", 1, 32, 32, 160, 160, 3, 5, 3, 0, 3),
}

"""Host side of the CTC loss: the public header's entry points, the argument checks of ``optim.ctc_loss`` (every refusal happens
before anything touches a device, so they run here), ``ctc_greedy_decode``, and the attention-maps remap on a checkpoint that
holds the auxiliary head's keys.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _ocr_ref as R
from worddiffusion_amd import _native as N
from worddiffusion_amd import ctc_greedy_decode
from worddiffusion_amd.optim import check_ctc_args, ctc_loss


def test_entry_points_and_limits():
    assert {"wd_ctc_loss", "wd_ctc_workspace_bytes"} <= set(N.header_symbols())
    assert N._SIGS["wd_ctc_workspace_bytes"] == (C.c_int64, [C.c_int, C.c_int, C.c_int])
    res, params = N._SIGS["wd_ctc_loss"]
    assert res is C.c_int and len(params) == 20 and params[11] is C.c_float
    # what the reference needs (T = 256, MAX_CHARS = 42) and what the issue asks for at the least
    assert N.DEFINES["WD_CTC_MAX_T"] >= 256 and N.DEFINES["WD_CTC_MAX_C"] >= 256 and N.DEFINES["WD_CTC_MAX_L"] >= 64
    lib = N.lib()  # (host arithmetic of the library: no HIP call)
    assert lib.wd_ctc_workspace_bytes(256, 64, 42) == 8 * 64 * (1 + 256 * (5 * 42 + 3))
    assert lib.wd_ctc_workspace_bytes(1, 1, 0) == 8 * (1 + 3)
    for T, B, L in ((0, 1, 1), (N.DEFINES["WD_CTC_MAX_T"] + 1, 1, 1), (8, 0, 1), (8, 1, -1), (8, 1, N.DEFINES["WD_CTC_MAX_L"] + 1)):
        assert lib.wd_ctc_workspace_bytes(T, B, L) == -1, (T, B, L)


def good():
    return dict(logits=torch.zeros(8, 2, 51), targets=torch.tensor([[1, 2, 3], [4, 5, 99]]), input_lengths=torch.tensor([8, 5]),
                target_lengths=torch.tensor([3, 2]))


def test_check_ctc_args_accepts():
    T, B, Cn, Lmax, tg, il, tl = check_ctc_args(**good())  # (the id 99 lies beyond its sample's length: not read)
    assert (T, B, Cn, Lmax) == (8, 2, 51, 3)
    assert tg.dtype == torch.int64 and il.dtype == torch.int32 and tl.dtype == torch.int32 and tg.is_contiguous()
    flat = dict(good(), targets=good()["targets"].reshape(-1))  # the reference's flattened token matrix
    assert torch.equal(check_ctc_args(**flat)[4], tg)
    empty = dict(good(), targets=torch.zeros(2, 0, dtype=torch.long), target_lengths=torch.tensor([0, 0]))
    assert check_ctc_args(**empty)[3] == 0


BAD = dict(
    logits_2d=dict(logits=torch.zeros(8, 51)),
    logits_double=dict(logits=torch.zeros(8, 2, 51, dtype=torch.float64)),
    logits_T_too_long=dict(logits=torch.zeros(N.DEFINES["WD_CTC_MAX_T"] + 1, 2, 3)),
    logits_C_too_wide=dict(logits=torch.zeros(8, 2, N.DEFINES["WD_CTC_MAX_C"] + 1)),
    logits_T_0=dict(logits=torch.zeros(0, 2, 51)),
    targets_float=dict(targets=torch.zeros(2, 3)),
    targets_wrong_batch=dict(targets=torch.zeros(3, 3, dtype=torch.long)),
    targets_too_long=dict(targets=torch.ones(2, N.DEFINES["WD_CTC_MAX_L"] + 1, dtype=torch.long)),
    id_negative=dict(targets=torch.tensor([[1, -1, 3], [4, 5, 6]])),
    id_C=dict(targets=torch.tensor([[1, 2, 3], [4, 51, 6]])),
    input_len_0=dict(input_lengths=torch.tensor([8, 0])),
    input_len_beyond_T=dict(input_lengths=torch.tensor([9, 5])),
    input_len_shape=dict(input_lengths=torch.tensor([8])),
    input_len_float=dict(input_lengths=torch.tensor([8.0, 5.0])),
    target_len_negative=dict(target_lengths=torch.tensor([3, -1])),
    target_len_beyond_Lmax=dict(target_lengths=torch.tensor([4, 2])),
    target_len_shape=dict(target_lengths=torch.tensor([[3, 2]])),
)


@pytest.mark.parametrize("name", sorted(BAD))
def test_ctc_loss_refuses_before_any_launch(name):
    """The tensors are host tensors: a refusal that came after the device check would be a NativeError, not a ValueError."""
    with pytest.raises(ValueError):
        ctc_loss(**dict(good(), **BAD[name]))


def test_ctc_loss_refuses_a_bad_scale_and_the_cpu():
    for s in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ctc_loss(**good(), scale=s)
    with pytest.raises(N.NativeError):  # valid arguments, host logits: there is no CPU path
        ctc_loss(**good())


def test_greedy_decode():
    T, Cn = 9, 5
    paths = [[0, 2, 2, 0, 2, 3, 3, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0], [4, 4, 4, 4, 0, 4, 1, 1, 1]]
    x = torch.full((T, 3, Cn), -1.0)
    for b, p in enumerate(paths):
        x[torch.arange(T), b, torch.tensor(p)] = 1.0
    assert ctc_greedy_decode(x) == [[2, 2, 3, 1], [], [4, 4, 1]]
    assert ctc_greedy_decode(x) == R.greedy_decode(x.numpy())
    assert ctc_greedy_decode(x, index2letter="ABCDE") == ["CCDB", "", "EEB"]
    assert ctc_greedy_decode(x, index2letter={1: "b", 2: "c", 3: "d", 4: "e"}) == ["ccdb", "", "eeb"]
    assert ctc_greedy_decode(x[:, 0]) == [[2, 2, 3, 1]]  # [T, C]: one sample
    rs = np.random.RandomState(0)
    y = rs.standard_normal((40, 4, 7)).astype(np.float32)
    assert ctc_greedy_decode(torch.from_numpy(y)) == R.greedy_decode(y)
    with pytest.raises(ValueError):
        ctc_greedy_decode(torch.zeros(4))


def test_attention_maps_remap_passes_the_head_s_keys_through():
    """A checkpoint of an ``attentionMaps=1, ocrTraining=1`` run holds ``auxhead.*`` (unet.py:1054-1092, 1468-1469) beside the
    renamed middle block: both directions of the remap leave those keys, their order and their tensors alone."""
    from worddiffusion_amd import remap_attention_maps_state_dict, to_attention_maps_state_dict
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    head = [f"auxhead.temporal_i.0.{k}" for k in ("weight", "bias")] + [f"auxhead.temporal_i.1.{k}" for k in bn]
    for i in range(3):
        head += [f"auxhead.temporal_m.{i}.0.{k}" for k in ("weight", "bias")] + [f"auxhead.temporal_m.{i}.1.{k}" for k in bn]
    head += [f"auxhead.{m}.{k}" for m in ("temporal_o", "lin1", "lin2") for k in ("weight", "bias")]
    saved = {"middle_block1.0.0.in_layers.0.weight": torch.zeros(2), "middle_block1.0.1.norm.weight": torch.ones(2),
             "middle_block1.1.0.in_layers.0.weight": torch.full((2,), 2.0), "out.2.bias": torch.full((2,), 3.0)}
    saved.update({k: torch.full((1,), float(i)) for i, k in enumerate(head)})
    ours = remap_attention_maps_state_dict(saved)
    assert list(ours) == ["middle_block.0.in_layers.0.weight", "middle_block.1.norm.weight", "middle_block.2.in_layers.0.weight",
                          "out.2.bias"] + head
    assert all(ours[k] is saved[k] for k in head)
    back = to_attention_maps_state_dict(ours)
    assert list(back) == list(saved) and all(back[k] is saved[k] for k in saved)

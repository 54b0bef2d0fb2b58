"""Growing the writer table on the host: ``model.add_writers`` on CPU models of both variants, the oracle on the grown table, and
the row-list validation of the row-wise kernels.  No GPU."""
import re

import pytest
import torch

from oracle import unet_oracle as U
from tests._common import SMALL, make_args
from worddiffusion_amd import UNetModel, UNetModelPhosc
from worddiffusion_amd import _native as N
from worddiffusion_amd.optim import check_rows
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs

VARIANTS = [("base", UNetModel), ("phosc", UNetModelPhosc)]
OLD, TED = SMALL["num_classes"], 4 * SMALL["model_channels"]


def model(cls, **over):
    m = cls(args=make_args(), **dict(SMALL, **over))
    fill_module_(m, 21)
    return m


@pytest.mark.parametrize("variant,cls", VARIANTS, ids=[v for v, _ in VARIANTS])
def test_add_writers_grows_the_table(variant, cls):
    m = model(cls)
    m._engine, m._train_engine = "stale", "stale"
    old = m.label_emb.weight.detach().clone()
    keys = list(m.state_dict())
    assert m.add_writers(2) == [OLD, OLD + 1]
    assert m._engine is None and m._train_engine is None  # nothing sized for the old table survives
    w = m.label_emb.weight
    assert isinstance(m.label_emb, torch.nn.Embedding) and isinstance(w, torch.nn.Parameter) and w.requires_grad
    assert m.num_classes == OLD + 2 and m.label_emb.num_embeddings == OLD + 2 and tuple(w.shape) == (OLD + 2, TED)
    assert torch.equal(w[:OLD].detach().view(torch.int32), old.view(torch.int32))
    mean = old.float().mean(0)
    assert torch.equal(w[OLD].detach(), mean) and torch.equal(w[OLD + 1].detach(), mean)
    assert m.add_writers(1, init=3) == [OLD + 2]
    assert torch.equal(m.label_emb.weight[OLD + 2].detach(), old[3])
    assert m.add_writers(2, init=[5, 0]) == [OLD + 3, OLD + 4]
    assert torch.equal(m.label_emb.weight[OLD + 3:].detach(), old[[5, 0]])
    t = torch.arange(3 * TED, dtype=torch.float32).reshape(3, TED) / 7
    assert m.add_writers(3, init=t) == [OLD + 5, OLD + 6, OLD + 7]
    assert torch.equal(m.label_emb.weight[OLD + 5:].detach(), t)
    assert torch.equal(m.label_emb.weight[:OLD].detach(), old)
    # the reference's key layout with the larger table: loads strictly into a model built with num_classes + k
    sd = m.state_dict()
    assert list(sd) == keys and tuple(sd["label_emb.weight"].shape) == (OLD + 8, TED)
    big = cls(args=make_args(), **dict(SMALL, num_classes=OLD + 8))
    big.load_state_dict(sd, strict=True)
    assert torch.equal(big.label_emb.weight.detach(), m.label_emb.weight.detach())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in big.named_parameters()]


@pytest.mark.parametrize("variant,cls", VARIANTS, ids=[v for v, _ in VARIANTS])
def test_add_writers_refusals(variant, cls):
    with pytest.raises(ValueError, match="num_classes"):
        model(cls, num_classes=None).add_writers(1)
    m = model(cls)
    before = m.label_emb
    for k in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="k must be"):
            m.add_writers(k)
    for init in (torch.zeros(2, TED + 1), torch.zeros(1, TED), torch.zeros(TED)):
        with pytest.raises(ValueError, match="init tensor"):
            m.add_writers(2, init=init)
    for init in (OLD, -1, [0, OLD], [0, -3]):
        with pytest.raises(ValueError, match="init id"):
            m.add_writers(2, init=init)
    for init in ([1], [1, 2, 3], "zeros", None, [0.5, 1.0]):
        with pytest.raises(ValueError, match="init must be"):
            m.add_writers(2, init=init)
    assert m.label_emb is before and m.num_classes == OLD  # a refused call changes nothing


@pytest.mark.parametrize("variant,cls", VARIANTS, ids=[v for v, _ in VARIANTS])
def test_oracle_accepts_the_grown_table(variant, cls):
    """The oracle's forward for a new id initialised from id a equals its forward for a."""
    m = model(cls)
    a = 6
    new = m.add_writers(1, init=a)[0]
    cfg = dict(SMALL, num_classes=OLD + 1)
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in U.state_dict_shapes(cfg, variant)}
    orc = U.UNetOracle(cfg, sd, variant, False)
    inp = synthetic_inputs(2, seed=8, hw=(4, 8), num_classes=OLD)
    y_new, y_old = torch.tensor([new, 2]), torch.tensor([a, 2])
    with torch.no_grad():
        out_new = orc(inp["x"].double(), inp["t"], inp["context"], y_new, None)
        out_old = orc(inp["x"].double(), inp["t"], inp["context"], y_old, None)
    assert torch.equal(out_new, out_old)


def test_row_list_validation():
    rmax = N.DEFINES["WD_ROWS_MAX"]
    with open(N.HEADER_PATH) as f:
        assert int(re.search(r"#define\s+WD_ROWS_MAX\s+(\d+)", f.read())[1]) == rmax == 64
    assert check_rows([3, 0, 7], 8) == (3, 0, 7)
    assert check_rows(torch.tensor([2, 1]), 3) == (2, 1)
    assert check_rows(range(rmax), rmax) == tuple(range(rmax))
    with pytest.raises(ValueError, match="distinct"):
        check_rows([1, 2, 1], 8)
    for rows in ([8], [-1], [0, 100]):
        with pytest.raises(ValueError, match=r"lie in \[0, 8\)"):
            check_rows(rows, 8)
    with pytest.raises(ValueError, match="1 .. 64"):
        check_rows([], 8)
    with pytest.raises(ValueError, match="1 .. 64"):
        check_rows(range(rmax + 1), 1000)
    for rows in ([1.0], [True], ["a"]):
        with pytest.raises(ValueError, match="integer"):
            check_rows(rows, 8)
    with pytest.raises(ValueError, match="sequence"):
        check_rows(5, 8)

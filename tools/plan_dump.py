"""Text dump of a launch plan, for comparing two commits: one line per op of P.cond, P.film, P.step, P.step1 (and P.bwd of a training
plan) with the function's name, its ``what`` and every argument.  Structures passed by reference are expanded field by field; every
device address is replaced by the ordinal of its first appearance in the dump, so two processes that build the same plan print the
same text.  Switches (WDIFF_*) are read from the environment as usual; engine attributes can be set with --set.

    python tools/plan_dump.py --cfg FULL --batch 48 --plan "film_steps=1000, mix=2"
    python tools/plan_dump.py --cfg SMALL --kind train --plan "label_drop=0.1" --run
    python tools/plan_dump.py --kind vae_enc"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _common as T  # noqa: E402
from worddiffusion_amd import UNetModel, UNetModelPhosc  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402
from worddiffusion_amd.synthetic import fill_module_, synthetic_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kind", default="step", choices=["step", "train", "vae_dec", "vae_enc"])
ap.add_argument("--cfg", default="FULL", choices=["FULL", "SMALL", "DEEP"])
ap.add_argument("--variant", default="base", choices=["base", "phosc"])
ap.add_argument("--phosc-len", type=int, default=0)
ap.add_argument("--depth", type=int, default=1, help="transformer_depth")
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--precision", default="bf16x3", choices=["bf16x3", "bf16"])
ap.add_argument("--hw", default="", help="latent map HxW (default: 8x32 for FULL, else 4x8)")
ap.add_argument("--plan", default="", help='keyword arguments of plan() / plan_train(), e.g. "film_steps=1000, attn_maps=True"')
ap.add_argument("--run", action="store_true", help="train: then one forward_train + backward on fixed inputs, SHA-256 of the results")
ap.add_argument("--set", default="", help='engine attributes, e.g. "fuse_xattn_pair=False"')
a = ap.parse_args()
kw = eval(f"dict({a.plan})")
dev = torch.device("cuda:0")
ids = {}


def value(v, ctype):
    if isinstance(v, C.Structure):
        return "{" + " ".join(f"{n}={value(getattr(v, n), t)}" for n, t in v._fields_) + "}"
    if isinstance(v, C.Array):
        return "[" + " ".join(value(e, v._type_) for e in v) + "]"
    if ctype is C.c_void_p:
        return "NULL" if not v else f"@{ids.setdefault(int(v), len(ids))}"
    return repr(v)


def dump(title, ops):
    print(f"---- {title}: {len(ops)} ops")
    for fn, args, what in ops:
        out = []
        for v, t in zip(args, fn.argtypes):  # (the stream, the last parameter, is not part of the plan)
            if isinstance(v, C.c_void_p):  # (a cast host address: the item records of wd_dw_group)
                v = v.value
            obj = getattr(v, "_obj", None)
            out.append(value(obj if obj is not None else v, t))
        print(f"{fn.__name__} | {what} | " + " ".join(out))
        # host-built tables in device memory: (position of the table's address, of its length, record type)
        tab = {"wd_colsum_finish_multi": (0, 1, N.WdColsumEntry), "wd_dw_group": (2, 3, N.WdDwItem)}.get(fn.__name__)
        if tab:
            dev_t = next(t for t in P.keep if isinstance(t, torch.Tensor) and t.data_ptr() == args[tab[0]])
            for e in (tab[2] * args[tab[1]]).from_buffer_copy(dev_t.cpu().numpy().tobytes()):
                print("    " + value(e, None))


if a.kind.startswith("vae"):
    from worddiffusion_amd.vae import AutoencoderKL
    m = fill_module_(AutoencoderKL(block_out_channels=(64, 128), layers_per_block=1, with_encoder=True), 1).to(dev).eval()
    eng = m.engine if a.kind == "vae_dec" else m.encoder_engine
else:
    cfg = dict(getattr(T, a.cfg), transformer_depth=a.depth)
    cls = UNetModel if a.variant == "base" else UNetModelPhosc
    m = fill_module_(cls(args=T.make_args(device="cuda:0", phosc=1 if a.phosc_len else 0), **cfg), 1).to(dev).eval()
    eng = m.train_engine if a.kind == "train" else m.engine
eng.set_precision(a.precision)
for k, v in eval(f"dict({a.set})").items():
    assert hasattr(eng, k), k
    setattr(eng, k, v)
eng.refresh_weights()
h, w = map(int, a.hw.split("x")) if a.hw else (8, 32) if a.cfg == "FULL" else (4, 8)
if a.kind == "vae_dec":
    P = eng.plan_decode(a.batch, h, w)
elif a.kind == "vae_enc":
    P = eng.plan_encode(a.batch, 8 * h, 8 * w)
elif a.kind == "train":
    P = eng.plan_train(a.batch, h, w, 10, a.phosc_len, **kw)
else:
    P = eng.plan(a.batch, h, w, 10, a.phosc_len, **kw)
for title in ("cond", "film", "step", "step1", "bwd"):
    if getattr(P, title, None):
        dump(title, getattr(P, title))
# the launches film_prepare issues per chunk of the table are held by the closure
for cell in getattr(P.film_prepare, "__closure__", None) or ():
    ops = cell.cell_contents
    if isinstance(ops, list) and ops and isinstance(ops[0], tuple) and callable(ops[0][0]):
        dump("film_prepare", ops)
if a.kind == "train":
    print(f"---- bwd_cuts: {P.bwd_cuts}")
    print(f"---- bwd_segments: {P.bwd_segments}")
if a.kind == "train" and a.run:
    # the engine sums in fixed orders (no float atomics), so both results are bit-stable
    inp = {k: v.to(dev) for k, v in synthetic_inputs(a.batch, seed=7, hw=(h, w), num_classes=cfg["num_classes"],
                                                     phosc_len=a.phosc_len).items()}
    eng.dropout_seed, eng.dropout_row_base = 1234, 0
    drop = kw.get("label_drop")
    if drop is None or drop == "mask":
        out = eng.forward_train(inp["x"], inp["t"], inp["context"], inp["y"], inp.get("phosc"),
                                writer_keep=None if drop is None else torch.arange(a.batch, device=dev) % 2 == 0)
        assert eng._live is P
    else:  # forward_train reaches only those two plans: the same calls on the plan dumped above
        eng.load_inputs(P, inp["x"], inp["t"], inp["context"], inp["y"], inp.get("phosc"), check=False)
        P.set_dropout_seed(eng.dropout_seed)
        P.set_row_base(eng.dropout_row_base)
        P.run_step(torch.cuda.current_stream(dev).cuda_stream)
        eng._live, out = P, P.out
    g = torch.Generator().manual_seed(11)
    eng.backward(torch.randn(out.shape, generator=g).to(dev), assign=False)
    torch.cuda.synchronize()
    for title, t in (("out", P.out), ("grad_arena", eng.grad_arena())):
        print(f"---- sha256 {title}: {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")

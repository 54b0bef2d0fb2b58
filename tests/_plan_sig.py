"""The kernel forms of a launch plan, without anything that merely grows with the batch: ``signature(engine, P)`` is one entry per
op of ``P.cond`` and ``P.step`` (the FiLM table ops, ``P.film`` and the closure of ``P.film_prepare``, are left out), ``diff`` says in
one line how two signatures differ.  Two batch sizes whose plans launch the same kernel forms in the same order have equal
signatures; tools/plan_thresholds.py scans the batch sizes at which they stop being equal.

An entry is (section, function name, ``what``, form).  The form is a readable string:
  wd_gemm       what wd_gemm_check resolves for the op's args - the launch family (wd_gemm_check_kernel), w_layout, tile, ksplit, nsrc -
                and which options are on: tickets (in-launch combine), slab (the slab form of the 64 x 320 kernel), slab_rows (the
                computed source rows), a32 (GroupNorm while staging), ln, gn, stat (GroupNorm statistics), f32 / planes (outputs)
  wd_ff_fused   front / no front, how proj_out rides along (folded / proj_out / none), whether tok2 is written, stat
  anything else the empty string: the function and its ``what`` are the form
No address, row count, pitch or byte count enters.

``train_signature(engine, P)`` is the same for a ``TrainPlan`` of ``engine.plan_train``: the sections are ``cond``, ``step`` and ``bwd``
(``P.bwd_cuts`` and ``P.bwd_segments`` are op indices and arena offsets: left out), with two more forms in the backward list:
  wd_dw         ntaps, hw_out, hw_src, npass, accumulate and the token slices the library will take: the args carry nslice = 0,
                so that is wd_dw_slices(m, n, c, ntaps), and with it the reduction path
  wd_dw_group   the number of layers in the launch, ntaps, hw_out, hw_src and wd_dw_group_slices(m, n, c, ntaps, items)"""
import ctypes as C

from worddiffusion_amd import _native as N

SLAB_BIT = N.GEMMW_SLAB_BIT  # wd_gemm_args.dbg of the RESOLVED args: the launch takes the slab form (include/wdiff_hip.h)


def _struct(args):
    """The structure an op passes by reference as its only argument."""
    return getattr(args[0], "_obj", args[0])


def gemm_form(lib, a) -> str:
    r = N.WdGemmArgs()
    if lib.wd_gemm_check(C.byref(a), C.byref(r)) != N.WD_OK:
        return "REFUSED by wd_gemm_check"
    kern = lib.wd_gemm_check_kernel(C.byref(a)).decode()
    flags = [name for name, on in (("tickets", r.tickets), ("slab", r.dbg & SLAB_BIT), ("slab_rows", r.slab_rows), ("a32", r.a32),
                                   ("ln", r.ln_gamma), ("gn", r.gn_gamma), ("stat", r.stat_part), ("f32", r.out_f32),
                                   ("planes", r.out_hi)) if on]
    return f"{kern} w_layout={r.w_layout} tile={r.tile} ksplit={r.ksplit} nsrc={r.nsrc} [{' '.join(flags)}]"


def ff_form(a) -> str:
    proj = "proj_out folded" if a.w32_hi else "proj_out" if a.w3_hi else "no proj_out"
    flags = ["front" if a.x_in else "no front", proj] + (["tok2 written"] if a.tok2 else []) + (["stat"] if a.stat_part else [])
    return ", ".join(flags)


def dw_form(lib, a) -> str:
    assert a.nslice == 0, "the plan fixes the slice count: the signature would have to say which"
    return (f"ntaps={a.ntaps} hw_out={a.hw_out} hw_src={a.hw_src} npass={a.npass} accumulate={a.accumulate} "
            f"slices={lib.wd_dw_slices(a.m, a.n, a.c, a.ntaps)}")


def dw_group_form(lib, a, nitems) -> str:
    assert a.nslice == 0, "the plan fixes the slice count: the signature would have to say which"
    return (f"items={nitems} ntaps={a.ntaps} hw_out={a.hw_out} hw_src={a.hw_src} "
            f"slices={lib.wd_dw_group_slices(a.m, a.n, a.c, a.ntaps, nitems)}")


def _signature(engine, P, sections) -> tuple:
    lib = engine.lib
    sig = []
    for section in sections:
        for fn, args, what in getattr(P, section):
            name = fn.__name__
            if name == "wd_gemm":
                form = gemm_form(lib, _struct(args))
            elif name == "wd_ff_fused":
                form = ff_form(_struct(args))
            elif name == "wd_dw":
                form = dw_form(lib, _struct(args))
            elif name == "wd_dw_group":
                form = dw_group_form(lib, _struct(args), int(args[3]))
            else:
                form = ""
            sig.append((section, name, what, form))
    return tuple(sig)


def signature(engine, P) -> tuple:
    return _signature(engine, P, ("cond", "step"))


def train_signature(engine, P) -> tuple:
    """``signature`` of a TrainPlan: forward lists and the backward list (the inference planner emits neither wd_dw form)."""
    return _signature(engine, P, ("cond", "step", "bwd"))


def families(sig) -> dict:
    """How often each kernel family is launched: {(function, family): count}; the family of a wd_gemm launch is its kernel
    (wd_gemm_check_kernel, without tile, K cut and options), that of a wd_ff_fused launch its whole form, else the function alone."""
    out = {}
    for _section, name, _what, form in sig:
        key = (name, form.split(" ")[0] if name == "wd_gemm" else form)
        out[key] = out.get(key, 0) + 1
    return out


def _keyed(sig) -> dict:
    """(section, what, occurrence) -> (function, form), in plan order: a ``what`` may repeat (one word_emb chain per token group)."""
    out, seen = {}, {}
    for section, name, what, form in sig:
        n = seen[(section, what)] = seen.get((section, what), 0) + 1
        out[(section, what, n)] = (name, form)
    return out


def _label(key) -> str:
    section, what, n = key
    return {"cond": "cond: ", "bwd": "bwd: "}.get(section, "") + what + (f" #{n}" if n > 1 else "")


def _names(keys) -> str:
    keys = list(keys)
    return ", ".join(_label(k) for k in keys[:3]) + (f" (+{len(keys) - 3} more)" if len(keys) > 3 else "")


def _show(entry) -> str:
    name, form = entry
    return f"{name} {form}" if form else name


def diff(sig_a, sig_b) -> str:
    """One line: the ops whose form changed grouped by (old form -> new form), then the ops only ``sig_a`` has (-) and the ops only
    ``sig_b`` has (+), grouped by function.  A group names its first three ops and counts the rest.  '' for equal signatures."""
    if tuple(sig_a) == tuple(sig_b):
        return ""
    ka, kb = _keyed(sig_a), _keyed(sig_b)
    changed, gone, new = {}, {}, {}
    for k, e in ka.items():
        if k not in kb:
            gone.setdefault(e[0], []).append(k)
        elif kb[k] != e:
            changed.setdefault((_show(e), _show(kb[k])), []).append(k)
    for k, e in kb.items():
        if k not in ka:
            new.setdefault(e[0], []).append(k)
    parts = [f"{_names(ks)}: {old} -> {to}" for (old, to), ks in changed.items()]
    parts += [f"- {fn} x{len(ks)}: {_names(ks)}" for fn, ks in gone.items()]
    parts += [f"+ {fn} x{len(ks)}: {_names(ks)}" for fn, ks in new.items()]
    if not parts:
        parts = ["same ops in another order"]
    return "; ".join(parts)


def read_scan(path) -> dict:
    """A scan file of tools/plan_thresholds.py -> {B: summary of the difference to B - 1}, in file order ('#' lines are comments)."""
    out = {}
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if not line.strip() or line.startswith("#"):
                continue
            head, sep, text = line.partition(": ")
            if not (head.startswith("B=") and head[2:].isdigit() and sep and text):
                raise ValueError(f"{path}: not a threshold line: {line[:80]!r}")
            if int(head[2:]) in out:
                raise ValueError(f"{path}: B = {head[2:]} is listed twice")
            out[int(head[2:])] = text
    return out


def release(engine):
    """Drops every plan the engine holds and returns their buffers to the device (a B = 48 plan holds about 1 GB).  A train
    engine also lets go of its training plans, of the plan the last forward left for ``backward`` and of the scratch sized for
    them; the gradient arena stays, so a ``param.grad`` handed out earlier stays valid."""
    import gc

    import torch
    engine._plans.clear()
    engine._cur_plan = None
    if hasattr(engine, "_tplans"):
        engine._tplans.clear()
        engine._live = None
        engine._scr = {k: v for k, v in engine._scr.items() if isinstance(k, tuple)}  # (as plan_train does between two shapes)
        engine._cs_scratch = None
    gc.collect()
    torch.cuda.empty_cache()


def signature_at(engine, B, phosc_len=0, h=8, w=32, ctx_len=10, planner=None) -> tuple:
    """The signature of the plan at batch ``B`` (plans only: nothing but ``refresh_weights`` launches); the plan is released.
    ``planner`` is the planner call, ``planner(B, h, w)`` -> Plan: ``engine.plan_decode`` (h, w of the latents) or ``engine.plan_encode``
    (h, w of the images) of a VAE engine; without it the forward's ``engine.plan(B, h, w, ctx_len, phosc_len)``."""
    engine.refresh_weights()
    sig = signature(engine, planner(B, h, w) if planner is not None else engine.plan(B, h, w, ctx_len, phosc_len))
    release(engine)
    return sig


def train_signature_at(engine, B, phosc_len=0, h=8, w=32, ctx_len=10) -> tuple:
    """``train_signature`` of ``engine.plan_train(B, h, w, ctx_len, phosc_len)`` (a TrainEngine); plans only, the plan is released."""
    engine.refresh_weights()
    sig = train_signature(engine, engine.plan_train(B, h, w, ctx_len, phosc_len))
    release(engine)
    return sig

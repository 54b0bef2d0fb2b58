"""ctypes binding of libwdiff_hip.so, derived at import from its public header (include/wdiff_hip.h): the Structure classes,
the argument types of every function and the WD_* constants are parsed from the header, so there is no second copy to keep in
step with it.

The product path has no CPU or eager-PyTorch fallback: if the shared library is missing or a symbol is
absent, importing/using it raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WDIFF_LIB") or os.path.join(_HERE, "libwdiff_hip.so")  # (WDIFF_LIB: A/B builds of the kernels)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "wdiff_hip.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "uint16_t": C.c_uint16, "uint8_t": C.c_uint8, "float": C.c_float, "double": C.c_double, "char": C.c_char}
_DECL = re.compile(r"(?:const\s+)?(\w+)(?:\s*(\*+)\s*|\s+)(\w+)((?:\s*,\s*\w+)*)\s*(?:\[(\d+)\])?")
_ITEMS = [re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;\s*"),  # struct: (body, name)
          re.compile(r"typedef\s+(\w+)\s+(\w+)\s*;\s*"),                        # alias: (known type, name)
          re.compile(r"([^;{}()]+)\(([^()]*)\)\s*;\s*")]                          # prototype: (result and name, parameters)


def parse_header(text: str):
    """The C subset include/wdiff_hip.h is written in -> (structs, prototypes, defines):
    structs     {C name: ctypes.Structure subclass} for every ``typedef struct [tag] { ... } name;``
    prototypes  {function: (restype, [(parameter name, ctype), ...])}
    defines     {name: value} for every integer ``#define WD_*``
    A pointer is c_void_p (callers pass ``tensor.data_ptr()`` or None), except ``char*`` (c_char_p) and, for a parameter, a
    pointer to a struct of the header (POINTER of its class).  Anything outside that subset raises ValueError: a header edit the
    binding would mistype must fail at import, not in a kernel."""
    types = dict(_SCALARS)
    structs, protos, defines, code = {}, {}, {}, []
    for line in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).splitlines():
        d = line.strip()
        m = re.fullmatch(r"#\s*define\s+(WD_\w+)\s+\(?\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\s*\)?", d)
        if m:
            defines[m[1]] = int(m[2], 0)
        elif not d.startswith("#"):
            code.append(line)
        elif not re.fullmatch(r"#\s*(ifn?def\s+\w+|endif|include\s*<\w+\.h>|define\s+(?!WD_)\w+)", d):
            raise ValueError(f"preprocessor line outside the header's grammar: {d!r}")
    code, wrapped = re.subn(r'extern\s+"C"\s*\{', "", "\n".join(code))
    code = code.strip()
    if wrapped:
        if not code.endswith("}"):
            raise ValueError('extern "C" { is not closed at the end of the header')
        code = code[:-1].rstrip()

    def decl(text, param):
        """``[const] type[*..] name[, name..][[n]]`` -> [(name, ctype), ...]"""
        m = _DECL.fullmatch(text.strip())
        if not m or (m[1] not in types and not (m[1] == "void" and m[2])):
            raise ValueError(f"declaration outside the header's grammar: {text.strip()!r}")
        base, stars, names = types.get(m[1]), m[2] or "", [m[3]] + re.findall(r"\w+", m[4])
        if not stars:
            t = base
        elif base is C.c_char and stars == "*":
            t = C.c_char_p
        elif param and stars == "*" and m[1] in structs:
            t = C.POINTER(base)
        else:
            t = C.c_void_p
        return [(n, t * int(m[5]) if m[5] else t) for n in names]

    pos = 0
    while pos < len(code):
        hit = next(((i, m) for i, m in enumerate(r.match(code, pos) for r in _ITEMS) if m), None)
        if hit is None:
            raise ValueError(f"declaration outside the header's grammar: {code[pos:pos + 80]!r}")
        kind, m = hit
        if kind == 0:
            fields = [f for part in m[1].split(";") if part.strip() for f in decl(part, False)]
            cls = type("".join(w.capitalize() for w in m[2].split("_")), (C.Structure,), {"_fields_": fields})
            types[m[2]] = structs[m[2]] = cls
        elif kind == 1:
            types[m[2]] = decl(f"{m[1]} {m[2]}", False)[0][1]
        else:
            params = [] if m[2].strip() == "void" else [decl(part, True)[0] for part in m[2].split(",")]
            (name, res), = decl(m[1], True)
            protos[name] = (res, params)
        pos = m.end()
    return structs, protos, defines


with open(HEADER_PATH) as _f:
    STRUCTS, _PROTOS, DEFINES = parse_header(_f.read())

WdSrc, WdGemmArgs, WdFfArgs, WdDwArgs, WdDwItem, WdDropout, WdRepackEntry, WdAdamwTableEntry, WdColsumEntry = (
    STRUCTS[n] for n in ("wd_src", "wd_gemm_args", "wd_ff_args", "wd_dw_args", "wd_dw_item", "wd_dropout", "wd_repack_entry",
                         "wd_adamw_table_entry", "wd_colsum_entry"))
WD_OK, WD_EINVAL, WD_ELAUNCH, WD_ESTATE = (DEFINES[n] for n in ("WD_OK", "WD_EINVAL", "WD_ELAUNCH", "WD_ESTATE"))
ACT_NONE, ACT_SILU, ACT_GEGLU = (DEFINES[n] for n in ("WD_ACT_NONE", "WD_ACT_SILU", "WD_ACT_GEGLU"))
# the bits of wd_gemm_args.dbg / wd_ff_args.dbg / wd_dw_args.dbg (kernel-form selectors of the parity tests and the benchmark tools)
DBG_NAMES = ("WD_DBG_STAMPS", "WD_DBG_STAGGER", "WD_DBG_FORCE_V4", "WD_DBG_FORCE_CONV3", "WD_DBG_FORCE_TICKETS", "WD_DBG_GEMMW_INSTEP",
             "WD_GEMMW_SLAB_OFF", "WD_GEMMW_SLAB_ON", "WD_EPI_BATCH_OFF", "WD_EPI_BATCH_ON", "WD_DBG_FORCE_V8")
(DBG_STAMPS, DBG_STAGGER, DBG_FORCE_V4, DBG_FORCE_CONV3, DBG_FORCE_TICKETS, DBG_GEMMW_INSTEP, GEMMW_SLAB_OFF, GEMMW_SLAB_ON, EPI_BATCH_OFF,
 EPI_BATCH_ON, DBG_FORCE_V8) = (DEFINES[n] for n in DBG_NAMES)
GEMMW_SLAB_BIT, EPI_BATCH_BIT = DEFINES["WD_GEMMW_SLAB_BIT"], DEFINES["WD_EPI_BATCH_BIT"]  # in the args a check returns: the form taken
VAE_MAX_LATENT, STREAM_VAE_POSTERIOR, STREAM_DROPOUT0, NCLASS = (
    DEFINES[n] for n in ("WD_VAE_MAX_LATENT", "WD_STREAM_VAE_POSTERIOR", "WD_STREAM_DROPOUT0", "WD_NCLASS"))
STREAM_KNOWN, TAG_KNOWN = DEFINES["WD_STREAM_KNOWN"], DEFINES["WD_TAG_KNOWN"]
STREAM_LABEL_DROP = DEFINES["WD_STREAM_LABEL_DROP"]
TAG_WALK, WALK_STEP, WALK_BLEND, WALK_JUMP = (DEFINES[n] for n in ("WD_TAG_WALK", "WD_WALK_STEP", "WD_WALK_BLEND", "WD_WALK_JUMP"))
CLASS_NAMES = ("gemm", "gn_stats", "gn_apply", "layernorm", "attention", "other", "gemm_other_tiles", "gemm_splitk_reduce",
               "gemm_two_per_cu", "gemm_weights_to_registers", "feed_forward_fused", "weight_gradient", "gemm_small_maps_whole_k")
assert len(CLASS_NAMES) == NCLASS, "CLASS_NAMES must name every profiling class of the header (WD_NCLASS)"

# Struct-pointer parameters the callers pass as a raw address rather than byref(): the item records of wd_dw_group live in a
# ctypes array on the host and in a tensor on the device.
_RAW_ADDRESS = {"wd_dw_group": ("items_host", "items_dev")}
assert all(p in dict(_PROTOS[f][1]) for f, ps in _RAW_ADDRESS.items() for p in ps)
_SIGS = {f: (res, [C.c_void_p if p in _RAW_ADDRESS.get(f, ()) else t for p, t in params])
         for f, (res, params) in _PROTOS.items()}


def header_symbols() -> list:
    """Every function the public header declares (used by the CPU test that the .so exports them all)."""
    return sorted(_PROTOS)


class NativeError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load (once) and type the shared library.  Raises if it is absent: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} is missing: build it with `python -m worddiffusion_amd.build` "
                          "(hipcc --offload-arch=gfx950); worddiffusion_amd has no CPU/eager fallback")
    l = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(l, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    for cname, cls in STRUCTS.items():  # a stale library beside a newer header (or the reverse)
        if cname + "_bytes" in _SIGS and getattr(l, cname + "_bytes")() != C.sizeof(cls):
            raise NativeError(f"{LIB_PATH}: {cname} is {getattr(l, cname + '_bytes')()} bytes in the library, {C.sizeof(cls)} in "
                              "worddiffusion_amd/_native.py - rebuild with `python -m worddiffusion_amd.build`")
    _lib = l
    return l


_ERR = {WD_EINVAL: "invalid argument", WD_ELAUNCH: "HIP launch/runtime error", WD_ESTATE: "bad call order"}


def check(rc: int, what: str) -> None:
    if rc != WD_OK:
        raise NativeError(f"{what} failed: {_ERR.get(rc, rc)}")

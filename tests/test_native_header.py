"""The ctypes binding is derived from include/wdiff_hip.h: the parser on a synthetic header, the derived layouts against what the
C compiler makes of the real header, and the three device-table records against their byte-level specification.  No GPU."""
import ctypes as C
import glob
import os
import re
import struct
import subprocess

import pytest

from worddiffusion_amd import _native as N
from worddiffusion_amd import dropout
from worddiffusion_amd.build import _hipcc

SYNTHETIC = """
/* A comment that spells a prototype: int wd_fake(int n); and a call wd_fake(int) - neither is a symbol. */
#ifndef FAKE_H
#define FAKE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define WD_ONE 1
#define WD_NEG (-7) /* trailing comment */
#define WD_HEX 0x100
typedef uint16_t wd_half;
typedef struct wd_inner {
    const wd_half* p; /* a const pointer */
    int32_t a, b, c;
    float f;
} wd_inner;
typedef struct {
    wd_inner pair[2];
    const wd_inner* next;
    uint64_t big;
    double d;
} wd_outer;
int wd_zero(void);
const char* wd_name(void);
int64_t wd_call(const wd_outer* o, wd_inner* out, const float* x, int n, uint32_t id, const char* tag,
                void** handle, void* stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_synthetic_header():
    structs, protos, defines = N.parse_header(SYNTHETIC)
    assert defines == {"WD_ONE": 1, "WD_NEG": -7, "WD_HEX": 256}
    assert list(structs) == ["wd_inner", "wd_outer"]
    inner, outer = structs["wd_inner"], structs["wd_outer"]
    assert (inner.__name__, outer.__name__) == ("WdInner", "WdOuter") and issubclass(inner, C.Structure)
    assert inner._fields_ == [("p", C.c_void_p), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("f", C.c_float)]
    assert [n for n, _ in outer._fields_] == ["pair", "next", "big", "d"]
    pair, nxt, big, d = (t for _, t in outer._fields_)
    assert pair._type_ is inner and pair._length_ == 2 and (nxt, big, d) == (C.c_void_p, C.c_uint64, C.c_double)
    assert C.sizeof(inner) == 24 and C.sizeof(outer) == 72
    assert sorted(protos) == ["wd_call", "wd_name", "wd_zero"]  # nothing from the comment
    assert protos["wd_zero"] == (C.c_int, []) and protos["wd_name"] == (C.c_char_p, [])
    res, params = protos["wd_call"]
    assert res is C.c_int64
    assert params == [("o", C.POINTER(outer)), ("out", C.POINTER(inner)), ("x", C.c_void_p), ("n", C.c_int), ("id", C.c_uint32),
                      ("tag", C.c_char_p), ("handle", C.c_void_p), ("stream", C.c_void_p)]


@pytest.mark.parametrize("bad", [
    "int wd_bad(size_t n);",                          # a type the binding has no mapping for
    "typedef struct wd_s { unsigned int n; } wd_s;",  # a two-word type
    "typedef struct wd_s { wd_later* p; } wd_s;",     # a pointer to a type not declared (yet)
    "int wd_bad(int (*callback)(int));",              # a prototype that does not split at its commas
    "int wd_bad(int);",                               # a parameter without a name
    "float *wd_a, *wd_b;",                            # not a typedef and not a prototype
    "#define WD_SHIFT (1 << 3)",                      # a WD_ constant that is not an integer literal
    "#if WD_ONE\n#endif",                             # a conditional the parser would have to evaluate
    'extern "C" {\nint wd_ok(void);',                 # the wrapper is not closed
])
def test_parser_raises_outside_its_grammar(bad):
    with pytest.raises(ValueError):
        N.parse_header("#include <stdint.h>\nint wd_before(void);\n" + bad + "\n")


def test_binding_is_the_header():
    """The public names are the parsed header: the classes, the re-exports, the constants and the size checks ``lib()`` makes."""
    with open(N.HEADER_PATH) as f:
        structs, protos, defines = N.parse_header(f.read())
    assert sorted(protos) == N.header_symbols() and set(N._SIGS) == set(protos)
    for name, (res, params) in protos.items():
        assert N._SIGS[name][0] is res and len(N._SIGS[name][1]) == len(params), name
    names = lambda ss: {c: [n for n, _ in s._fields_] for c, s in ss.items()}  # noqa: E731
    assert names(structs) == names(N.STRUCTS)
    assert N.STRUCTS["wd_gemm_args"] is N.WdGemmArgs and N.STRUCTS["wd_repack_entry"] is N.WdRepackEntry
    assert dropout.WdDropout is N.STRUCTS["wd_dropout"] and dropout.STREAM_DROPOUT0 == defines["WD_STREAM_DROPOUT0"] == 0x100
    assert (N.WD_OK, N.WD_EINVAL, N.WD_ELAUNCH, N.WD_ESTATE) == (0, -1, -2, -3)
    assert (N.ACT_NONE, N.ACT_SILU, N.ACT_GEGLU, N.NCLASS) == (0, 1, 2, len(N.CLASS_NAMES))
    # wd_gemm takes its arguments by reference, the tables of wd_dw_group travel as addresses
    assert N._SIGS["wd_gemm"] == (C.c_int, [C.POINTER(N.WdGemmArgs), C.c_void_p])
    assert N._SIGS["wd_dw_group"] == (C.c_int, [C.POINTER(N.WdDwArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    sized = sorted(c for c in N.STRUCTS if c + "_bytes" in N._SIGS)
    assert sized == ["wd_adamw_table_entry", "wd_colsum_entry", "wd_dw_args", "wd_dw_item", "wd_ff_args", "wd_gemm_args",
                     "wd_repack_entry"]
    lib = N.lib()
    for c in sized:
        assert getattr(lib, c + "_bytes")() == C.sizeof(N.STRUCTS[c]), c


def test_layout_against_the_compiler(tmp_path):
    """sizeof / offsetof of every field of every header struct, as the host C compiler sees the header (plain C, <stdint.h>
    only), against the derived Structures."""
    lines = ['#include "wdiff_hip.h"', "#include <stddef.h>", "#include <stdio.h>", "int main(void) {"]
    want = []
    for cname, cls in N.STRUCTS.items():
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        want.append(f"{cname} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            lines.append(f'    printf("{cname}.{field} %zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname}*)0)->{field}));')
            want.append(f"{cname}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    lines += ["    return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    include = N.HEADER_PATH.rsplit("/", 1)[0]
    subprocess.run([_hipcc(), "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", include, str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(want) > 170 and got == want


REPACK = [  # src0, src1, dst_hi, dst_lo, N, C, T, mode, npad, ld, g, ntile_c, chunk0, row_off, col_off
    (0x7f0000001000, 0x7f0000002000, 0x7f0000003000, 0x7f0000003800, 320, 640, 9, 0, 0, 5760, 0, 20, 0, 0, 0),
    (0x7f0000001000, 0, 0x7f0000004000, 0, 1280, 1, 1, 2, 0, 0, 16, 1, 2 ** 32 + 17, 0, 0),       # null src1, chunk0 > 2**32
    (2 ** 64 - 8, 0, 1, 2, 2560, 320, 1, 3, 0, 2560, 16, 10, 2 ** 40, -64, 318),                   # negative row_off
]
ADAMW = [  # p, g, m, v, ema, n, chunk0
    (0x7f0000001000, 0x7f0000002000, 0x7f0000003000, 0x7f0000004000, 0x7f0000005000, 1, 0),
    (0x7f0000001000, 0, 0x7f0000003000, 0x7f0000004000, 0, 2 ** 31 + 5, 2 ** 32 + 3),              # null g and ema
    (2 ** 64 - 4, 1, 2, 3, 4, 2 ** 62, -1),
]
COLSUM = [  # part, out, nblk, c, ld, accumulate, scale, pad
    (0x7f0000001000, 0x7f0000002000, 64, 320, 320, 0, 1.0, 0),
    (2 ** 64 - 4, 0, 1, 1, 2 ** 31 - 1, 1, -0.375, 0),
    (0, 0x7f0000002000, 1024, 2560, 2560, 1, 3.0e38, -1),
]


@pytest.mark.parametrize("cls,fmt,size,rows", [("WdRepackEntry", "<QQQQiiiiiiiiqii", 80, REPACK),
                                               ("WdAdamwTableEntry", "<QQQQQqq", 56, ADAMW),
                                               ("WdColsumEntry", "<QQiiiifi", 40, COLSUM)])
def test_table_records_byte_for_byte(cls, fmt, size, rows):
    """The format strings are the specification of the device-table records (what the kernels of csrc/wd_pack.hip,
    wd_train.hip and wd_bwd.hip index): a record and an array of records built from the header must be those bytes."""
    rec = getattr(N, cls)
    assert C.sizeof(rec) == struct.calcsize(fmt) == size
    for row in rows:
        assert bytes(rec(*row)) == struct.pack(fmt, *row), row
    assert bytes((rec * len(rows))(*rows)) == b"".join(struct.pack(fmt, *row) for row in rows)


SELECTORS = N.DBG_NAMES  # every bit of wd_gemm_args.dbg / wd_ff_args.dbg / wd_dw_args.dbg a caller may set or a check returns


def test_form_selectors_are_named_once_in_the_header():
    """Each selector is one bit of its own; the resolved *_BIT of a switch is its *_ON request bit."""
    values = [N.DEFINES[n] for n in SELECTORS]
    assert all(v > 0 and v & (v - 1) == 0 for v in values), dict(zip(SELECTORS, values))
    assert len(set(values)) == len(values) == 11
    for switch in ("WD_GEMMW_SLAB", "WD_EPI_BATCH"):
        assert N.DEFINES[switch + "_BIT"] == N.DEFINES[switch + "_ON"] != N.DEFINES[switch + "_OFF"]
    assert (N.GEMMW_SLAB_BIT, N.EPI_BATCH_BIT, N.DBG_STAMPS) == (N.GEMMW_SLAB_ON, N.EPI_BATCH_ON, N.DEFINES["WD_DBG_STAMPS"])


def test_no_selector_literal_left_in_python():
    """A plain text search: no line of the package, the tests or the tools that speaks of the selector word still carries a
    hexadecimal literal - the values live in include/wdiff_hip.h alone."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    word, literal = "dbg", re.compile(r"0[xX][0-9a-fA-F]")
    hits = []
    for sub in ("worddiffusion_amd", "tests", "tools"):
        for path in sorted(glob.glob(os.path.join(root, sub, "**", "*.py"), recursive=True)):
            with open(path) as f:
                hits += [f"{os.path.relpath(path, root)}:{i}" for i, line in enumerate(f, 1) if word in line and literal.search(line)]
    assert not hits, hits

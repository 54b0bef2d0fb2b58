"""Text dump of what wd_gemm's planner decides, for comparing two builds of the library: a fixed grid of wd_gemm_args goes through
wd_gemm_check / wd_gemm_check_kernel and every case prints one line - its id, the return code, the launch family and the resolved
args (every number; NULL or SET for every pointer).  Nothing is launched and no GPU is needed: every operand address is a
placeholder the planner never reads through.  The library is the one WDIFF_LIB names (default: the tree's); the WDIFF_* switches
are read by the library as usual, once per process, so one process per switch setting.

    WDIFF_LIB=/other/tree/worddiffusion_amd/libwdiff_hip.so python tools/gemm_resolve_dump.py > other.txt
    WDIFF_GEMM_V4=0 python tools/gemm_resolve_dump.py --summary        # counts per family, refusals, what each dbg selector moved"""
import collections
import ctypes as C
import itertools
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from worddiffusion_amd import _native as N  # noqa: E402

P = 1 << 20  # placeholder operand address: non-NULL, 16-byte aligned
WS = 128 * 128 * 160 * 8  # workspace floats
LIN = lambda c: ("lin%d" % c, lambda hw, w: [(c, 1, False, 0)], {})  # noqa: E731
SOURCES = [
    LIN(32), LIN(64), LIN(96), LIN(320),
    ("same3", lambda hw, w: [(320, 9, True, hw)], {}),
    ("stride2", lambda hw, w: [(320, 9, True, 4 * hw)], {}),
    ("same3+skip", lambda hw, w: [(320, 9, True, hw), (640, 1, False, 0)], {}),
    ("phase4", lambda hw, w: [(640, 4, True, max(hw // 4, 1))], dict(w_ngroups=4, w_group_stride=320 * 4 * 640)),
    ("a32", lambda hw, w: [(320, 1, False, hw)], dict(a32=P, a32_ld=320, a32_part=P, a32_nchunk=4, a32_pcpg=10, a32_cpg=10, a32_gamma=P,
                                                      a32_beta=P)),
]
# (m, hw_out, image width): ragged m, one-tile grids, whole samples of 256 / 64 / 16 / 1 positions
SHAPES = [(64 * 256, 256, 32), (64 * 64, 64, 16), (8 * 64, 64, 16), (130, 1, 1), (64, 64, 16), (200, 16, 4), (128 * 256, 256, 32)]
NS = [320, 640, 2560, 160, 128, 100, 90, 81]
TILES = [0, 128064, 128160, 128128, 64064, 64320, 64080, 96096]
PLANES = dict(out_hi=P, out_lo=P)
OPTIONS = {
    "plain": {},
    "silu": dict(act=N.ACT_SILU),
    "geglu": dict(act=N.ACT_GEGLU),
    "npass1": dict(npass=1),
    "npass2": dict(npass=2),
    "planes": dict(PLANES),
    "bias+rowvec+resid": dict(bias=P, rowvec=P, resid=P),
    "resid_rows": dict(resid=P, resid_rows=P),
    "stat": dict(stat_part=P, stat_cpg=10),
    "stat cpg 20": dict(stat_part=P, stat_cpg=20),
    "stat cpg 7": dict(stat_part=P, stat_cpg=7),
    "stat, out_f32 off grid": dict(stat_part=P, stat_cpg=10, out_f32=P + 4),
    "stat+gn": dict(stat_part=P, stat_cpg=10, gn_gamma=P, gn_beta=P, gn_cpg=20, gn_silu=1, **PLANES),
    "stat+gn, gamma off grid": dict(stat_part=P, stat_cpg=10, gn_gamma=P + 4, gn_beta=P, gn_cpg=20, **PLANES),
    "ln": dict(ln_gamma=P, ln_beta=P, **PLANES),
    "ln, out_hi off grid": dict(ln_gamma=P, ln_beta=P, out_hi=P + 2, out_lo=P),
    "groups, stride off grid": dict(w_group_stride=320 * 4 * 640 + 4),
    "no out": dict(out_f32=None),
    "no w_lo": dict(w_lo=None),
}
DBG = [n for n in N.DBG_NAMES if n != "WD_DBG_STAGGER"]  # (WD_DBG_STAGGER is a resolved bit, not a selector)


def gemm_args(m, n, hw_out, srcs, **fields):
    """srcs: (c, ntaps, gathered, hw_src) per source; every pointer a placeholder; pitches = widths unless `fields` says otherwise."""
    a = N.WdGemmArgs()
    for i, (c, ntaps, gathered, hw_src) in enumerate(srcs):
        s = a.src[i]
        s.hi = s.lo = P
        s.gather = P if gathered else None
        s.ld, s.c, s.ntaps, s.hw_src = c, c, ntaps, hw_src
    a.nsrc, a.npass, a.w_hi, a.w_lo = len(srcs), 3, P, P
    a.m, a.n, a.ktot, a.hw_out = m, n, sum(c * t for c, t, _, _ in srcs), hw_out
    nout = n // 2 if fields.get("act") == N.ACT_GEGLU else n
    a.out_f32, a.out_ld, a.ws, a.ws_floats = P, nout, P, WS
    a.out_pl_ld = nout if fields.get("out_hi") else 0
    a.resid_ld = nout if fields.get("resid") else 0
    a.rowvec_ld = nout if fields.get("rowvec") else 0
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def cases():
    """(id, args) in a fixed order."""
    def one(tag, src, shape, n, **fields):
        name, make, extra = src
        m, hw, width = shape
        f = dict(extra)
        if fields.get("w_layout", 0) != 3:  # (a32 and weight groups exist for w_layout 3 only: elsewhere the plain source)
            f = {}
        f.update(fields)
        if name in ("same3", "stride2", "same3+skip"):
            f.setdefault("slab_rows", width // 2 if name == "stride2" and width > 1 else width)
        cid = f"{tag} {name} m{m} hw{hw} n{n} " + " ".join(f"{k}={'SET' if v == P else v}" for k, v in sorted(fields.items()) if k != "dbg")
        return cid.strip(), gemm_args(m, n, hw, make(hw, width), **f)

    # 1. source x shape x n x w_layout x tile, the K cut left to the planner
    for src, shape, n, wl, tile in itertools.product(SOURCES, SHAPES[:6], NS, (0, 1, 2, 3, 5), TILES):
        yield one("grid", src, shape, n, w_layout=wl, tile=tile)
    # 2. the K cut, the workspace and the tickets
    for src, shape, n, wl, tile in itertools.product(SOURCES[3:7], SHAPES, (320, 640, 160), (0, 2, 3), (0, 128160, 128064, 64320)):
        for ks, ws, tk in itertools.product((0, 1, 2, 4, N.DEFINES["WD_MAX_KSPLIT"] + 1), ("ws", "no ws", "small ws"), (False, True)):
            f = dict(w_layout=wl, tile=tile, ksplit=ks)
            if ws == "no ws":
                f.update(ws=None, ws_floats=0)
            elif ws == "small ws":
                f.update(ws_floats=shape[0] * n)
            if tk:
                f.update(tickets=P, ntickets=4096)
            yield one("cut", src, shape, n, **f)
    # 3. activation, npass, statistics / GroupNorm / LayerNorm / weight groups, each also misaligned
    for (oname, opt), src, shape, n, (wl, tile) in itertools.product(
            OPTIONS.items(), SOURCES[3:], SHAPES[:3], (320, 640, 2560),
            ((0, 0), (0, 128160), (0, 128064), (2, 0), (3, 0), (3, 64320), (3, 64080), (3, 128160), (1, 0))):
        yield one(f"opt[{oname}]", src, shape, n, w_layout=wl, tile=tile, **opt)
    # 4. every dbg selector alone (and none), over launches of every family
    for sel, src, shape, n, (wl, tile), ks in itertools.product(
            [None] + DBG, SOURCES[3:7], SHAPES[:4] + SHAPES[6:], (320, 640),
            ((0, 0), (0, 128160), (2, 128160), (2, 0), (3, 64320), (3, 64080), (1, 0)), (0, 2)):
        f = dict(w_layout=wl, tile=tile, ksplit=ks, tickets=P, ntickets=4096)
        if sel:
            f["dbg"] = N.DEFINES[sel]
        yield one(f"dbg[{sel}]", src, shape, n, **f)
    # 5. long K over a handful of tiles (the token reductions of the training step), where the cap of the automatic K cut binds
    for c, m, n, (wl, tile) in itertools.product((4096, 16384), (320, 640), (320, 640), ((0, 0), (0, 128160), (0, 64064), (3, 64320), (3, 0))):
        yield one("longk", LIN(c), (m, 1, 1), n, w_layout=wl, tile=tile)


def fields_text(v):
    out = []
    for name, t in v._fields_:
        x = getattr(v, name)
        if isinstance(x, C.Array):
            out.append(f"{name}=[" + " ".join("{" + fields_text(e) + "}" for e in x) + "]")
        elif t is C.c_void_p or isinstance(x, (C._Pointer, type(None))):
            out.append(f"{name}={'SET' if x else 'NULL'}")
        else:
            out.append(f"{name}={x!r}")
    return " ".join(out)


def main():
    summary = "--summary" in sys.argv
    lib = N.lib()
    lines = []
    for cid, a in cases():
        out = N.WdGemmArgs()
        rc = lib.wd_gemm_check(C.byref(a), C.byref(out))
        fam = lib.wd_gemm_check_kernel(C.byref(a))
        fam = fam.decode() if fam else "-"
        lines.append((cid, f"{cid} | rc={rc} | {fam}" + (" | " + fields_text(out) if rc == N.WD_OK else "")))
    if not summary:
        print("\n".join(line for _, line in lines))
        return
    fams = collections.Counter(line.split(" | ")[2] for _, line in lines)
    print(f"{len(lines)} cases, {fams['-']} refused ({100.0 * fams['-'] / len(lines):.1f} %), experimental build: {lib.wd_gemm_experimental()}")
    for fam, cnt in sorted(fams.items()):
        print(f"  {fam}: {cnt}")
    # (the selector is in the tag of a case id only: what follows the tag names the launch)
    base = {cid[len("dbg[None]"):]: line.split(" | ", 1)[1] for cid, line in lines if cid.startswith("dbg[None]")}
    for sel in DBG:
        tag, bit = f"dbg[{sel}]", N.DEFINES[sel]
        strip = lambda s: re.sub(r" dbg=(\d+)", lambda mo: f" dbg={int(mo.group(1)) & ~bit}", s)  # noqa: E731  (not the echoed bit alone)
        pairs = [(base[cid[len(tag):]], line.split(" | ", 1)[1]) for cid, line in lines if cid.startswith(tag)]
        print(f"  {sel}: {sum(p != q for p, q in pairs)} of {len(pairs)} cases differ from the same launch without it, "
              f"{sum(strip(p) != strip(q) for p, q in pairs)} in more than that bit of the resolved dbg")


if __name__ == "__main__":
    main()

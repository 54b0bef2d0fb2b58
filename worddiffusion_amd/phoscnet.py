"""The PHOSCnet word recogniser on the HIP kernels of this package, and the verifier the bulk pipelines end a batch with.

Reference: ``ResPhoSCNetZSL/modules/models.py:15-80`` (``PHOSCnet``: thirteen 3x3 convolutions + ReLU with two 2x2 max-pools,
``TemporalPyramidPooling([1, 2, 5])`` to 4096 features, two three-layer MLP heads - 165 PHOS counts behind a ReLU, 604 PHOC bits
behind a sigmoid) and ``modules/engine.py:130-146`` (zero-shot recognition: the cosine of the predicted 769-vector against the
PHOSC vector of every word of a lexicon, first maximum wins).  The 769-vector is the one ``UNetModelPhosc`` is conditioned on
(``phosc.phosc_batch`` builds it from a word); the 4096 pooled features are what ``wrd_proj = nn.Linear(4096, 320)`` of the base
checkpoints takes.

Inference only: every convolution and linear layer is ``wd_gemm`` (split-bf16 operands, three passes), the ReLUs live in the
streaming stage between two GEMMs (``wd_relu_pool_planes`` - never in a GEMM epilogue), then ``wd_tpp_max``, ``wd_phosc_finish``
and ``wd_phosc_score`` (csrc/wd_phoscnet.hip).  Training mode raises: nn.Dropout makes the training forward another function,
and there is no backward.  There is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _native as N
from .engine import Act, GemmForm, Plan, RecipeBook, UNetEngine, _Recipe

# models.py:19-48: (in, out) of a convolution, "P" = nn.MaxPool2d((2, 2), stride=2); every convolution is followed by nn.ReLU
CONV_STACK = ((3, 64), (64, 64), "P", (64, 128), (128, 128), "P", (128, 256), (256, 256), (256, 256), (256, 256), (256, 256),
              (256, 256), (256, 512), (512, 512), (512, 512))
TPP_LEVELS = (1, 2, 5)
N_FEAT, N_PHOS, N_PHOC = 512 * sum(TPP_LEVELS), 165, 604
N_PHOSC = N_PHOS + N_PHOC


def _conv_stack() -> nn.Sequential:
    mods: List[nn.Module] = []
    for item in CONV_STACK:
        if item == "P":
            mods.append(nn.MaxPool2d((2, 2), stride=2))
        else:
            mods += [nn.Conv2d(item[0], item[1], (3, 3), padding="same"), nn.ReLU()]
    return nn.Sequential(*mods)


def _head(n_out: int, last: nn.Module) -> nn.Sequential:
    return nn.Sequential(nn.Linear(N_FEAT, 4096), nn.ReLU(), nn.Dropout(), nn.Linear(4096, 4096), nn.ReLU(), nn.Dropout(),
                         nn.Linear(4096, n_out), last)


def conv_layers(net: "PHOSCnet") -> List[Tuple[int, nn.Conv2d, bool]]:
    """(index in ``net.conv``, the convolution, a max-pool stands before it) in execution order."""
    out, pool = [], False
    for i, m in enumerate(net.conv):
        if isinstance(m, nn.MaxPool2d):
            pool = True
        elif isinstance(m, nn.Conv2d):
            out.append((i, m, pool))
            pool = False
    return out


class PHOSCnet(nn.Module):
    """The reference's ``state_dict`` keys and shapes (``conv.{0,2,5,...,26}``, ``phos.{0,3,6}``, ``phoc.{0,3,6}``): a reference
    checkpoint loads with ``strict=True``.  ``forward`` / ``features`` / ``phosc`` take [B, 3, H, W] float images in [0, 1] on the
    GPU, any H >= 4, W >= 4."""

    CHUNK = 16  # images per launch plan: a larger batch runs as replays of it (a plan holds every buffer of its batch)

    def __init__(self):
        super().__init__()
        self.conv = _conv_stack()
        self.phos = _head(N_PHOS, nn.ReLU())
        self.phoc = _head(N_PHOC, nn.Sigmoid())
        self.chunk = self.CHUNK
        self._engine: Optional[PhoscNetEngine] = None
        self.eval()

    @property
    def engine(self) -> "PhoscNetEngine":
        if self._engine is None:
            self._engine = PhoscNetEngine(self)
        return self._engine

    def _run(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        if self.training:
            raise NotImplementedError("PHOSCnet runs in eval mode only: nn.Dropout makes the training forward another function and "
                                      "there is no backward (call .eval())")
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] == 0:
            raise ValueError(f"images must be [B, 3, H, W], got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        if x.shape[2] < 4 or x.shape[3] < 4:
            raise ValueError(f"image height and width must be at least 4 (two 2x2 max-pools), got {tuple(x.shape)}")
        if not x.is_floating_point():
            raise ValueError(f"images must be floating point in [0, 1] (WordVerifier.prepare converts uint8), got {x.dtype}")
        if x.requires_grad:
            raise NotImplementedError("PHOSCnet has no backward: pass images that do not require grad")
        if not x.is_cuda:
            raise N.NativeError("worddiffusion_amd runs on an MI355X only: move the images and the PHOSCnet to cuda "
                                "(there is no CPU / eager fallback)")
        return self.engine.run(x.detach().float().contiguous(), max(1, int(self.chunk)))

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = self._run(x)["phosc"]
        return {"phos": out[:, :N_PHOS], "phoc": out[:, N_PHOS:]}

    @torch.no_grad()
    def features(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 4096]: the pooled features (``temporal_pool`` of ``conv``), the input of both heads."""
        return self._run(x)["features"]

    @torch.no_grad()
    def phosc(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 769] = relu(phos) | sigmoid(phoc): ``torch.cat((vector_dict['phos'], vector_dict['phoc']), dim=1)`` (engine.py:131)."""
        return self._run(x)["phosc"]

    @torch.no_grad()
    def outputs(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Everything a call makes: ``features`` [B, 4096], ``phosc`` [B, 769] and both heads' pre-activation rows ``phos_logits``
        [B, 165] / ``phoc_logits`` [B, 604] (what the parity tests compare)."""
        return self._run(x)


class PhoscNetEngine(UNetEngine):
    """Launch plan of PHOSCnet out of the UNet engine's building blocks: im2col + GEMM for the 3-channel first convolution,
    tap-gather GEMMs (3x3 / pad 1) for the other twelve, ``wd_relu_pool_planes`` between two GEMMs, ``wd_tpp_max``, the six linear
    layers as GEMMs over per-sample rows (``phos.0`` and ``phoc.0`` as one 8192-row matrix), ``wd_phosc_finish``.

    A plan keeps every buffer of its batch, so ``run`` takes a batch as replays of a plan of at most ``chunk`` images (plus one
    smaller plan for a remainder); plans are cached per (B, H, W)."""

    def __init__(self, model: PHOSCnet):
        super().__init__(model, "phoscnet")
        self._levels = (C.c_int32 * len(TPP_LEVELS))(*TPP_LEVELS)

    # ---- operands -----------------------------------------------------------------------------------------------------
    def _head_rows(self, n: int) -> int:
        """Rows of the last layer's weight matrix: n where wd_gemm takes a GEMM with n output columns over per-sample rows, else
        n zero-padded to the next multiple of 64 (wd_phosc_finish reads the real columns)."""
        a = N.WdGemmArgs()
        a.src[0].hi = a.src[0].lo = 16  # (placeholders: wd_gemm_check reads no memory)
        a.src[0].ld = a.src[0].c = 4096
        a.src[0].ntaps = 1
        a.nsrc, a.npass, a.m, a.n, a.ktot, a.hw_out = 1, self.npass, 16, n, 4096, 1
        a.w_hi = a.w_lo = a.out_f32 = a.bias = 16
        a.out_ld = n
        return n if self.lib.wd_gemm_check(C.byref(a), None) == N.WD_OK else ((n + 63) // 64) * 64

    def _recipes(self) -> RecipeBook:
        m = self.model
        R = RecipeBook()
        self.kpad_in = 32  # 9 taps x 3 channels, padded to the GEMM's 32-column K step
        for i, conv, _ in conv_layers(m):
            name = f"c{i}"
            if conv.in_channels == 3:
                R.matrix(name + ".w", conv.out_channels, self.kpad_in).fwd(conv.weight)
            else:
                R.matrix(name + ".w", conv.out_channels, 9 * conv.in_channels).fwd(conv.weight)
            R.vector(name + ".b", conv.bias)
        # phos.0 | phoc.0 read the same features: one matrix, one launch
        R.matrix("h0.w", 2 * 4096, N_FEAT).fwd(m.phos[0].weight).fwd(m.phoc[0].weight, row_off=4096)
        R.vector_cat("h0.b", [m.phos[0].bias, m.phoc[0].bias])
        self._rows = {}
        for tag, head, n in (("phos", m.phos, N_PHOS), ("phoc", m.phoc, N_PHOC)):
            R.linear(tag + ".3", head[3])
            rows = self._rows[tag] = self._head_rows(n)
            R.matrix(tag + ".6.w", rows, 4096).fwd(head[6].weight)   # (rows past n stay zero)
            r = R[tag + ".6.b"] = _Recipe(tag + ".6.b", False, shape=(rows,))
            r.vec(head[6].bias)
        return R

    def _gemm_form(self, a, srcs, whole_w: bool, w_row_off: int) -> GemmForm:
        """The shared policy, then wd_gemm_check's word on it at THIS shape: a form it refuses falls back to the generic gather
        form; a GEMM wd_gemm refuses altogether fails here, while the plan is built."""
        form = super()._gemm_form(a, srcs, whole_w, w_row_off)
        if form.fields and self._resolved(a, **form.fields) is None:
            form = GemmForm("generic", {})
        if not form.fields and self._resolved(a) is None:
            raise N.NativeError(f"wd_gemm refuses the {a.m} x {a.n} x {a.ktot} GEMM of PHOSCnet (wd_gemm_check)")
        return form

    # ---- plan ---------------------------------------------------------------------------------------------------------
    def _relu_planes(self, P: Plan, what: str, x: Act, pool: int) -> Tuple[torch.Tensor, int, int]:
        """nn.ReLU (+ the 2x2 max-pool) of the fp32 map -> the operand planes of the next GEMM and their (h, w)."""
        B = self._B
        h, w = (x.h // 2, x.w // 2) if pool == 2 else (x.h, x.w)
        pl = self._planes(P, B * h * w, x.c)
        P.step.append((self.lib.wd_relu_pool_planes, (x.t.data_ptr(), x.c, B, x.h, x.w, x.c, pool, *self._hilo(pl), x.c), what))
        return pl, h, w

    def plan_forward(self, B: int, H: int, W: int) -> Plan:
        key = ("phoscnet", B, H, W, self.npass)
        P = self._cached_plan(self._plans, key)
        if P is not None:
            return P
        m, lib, dev = self.model, self.lib, self.device
        P = self._begin_plan(Plan(), B)
        step = P.step
        P.x_in = torch.zeros((B, 3, H, W), dtype=torch.float32, device=dev)
        cur = None
        for i, conv, pool in conv_layers(m):
            name = f"c{i}"
            if cur is None:
                cur, _ = self._head_gemm(P, step, "conv.0", P.x_in, name, label="im2col(x)", want_stats=False)
                continue
            pl, h, w = self._relu_planes(P, f"conv.{i}: relu" + ("+maxpool" if pool else "") + " -> planes", cur, 2 if pool else 1)
            out = self._f32(P, B * h * w, conv.out_channels)
            self._gemm(step, f"conv.{i}", [self._src(pl, conv.in_channels, 9, self._table(h, w, "same"), h * w)], name + ".w",
                       B * h * w, h * w, bias=self._w[name + ".b"], out_f32=out, out_ld=conv.out_channels, want_stats=False)
            cur = Act(out, conv.out_channels, h, w)
        P.feat = self._f32(P, B, N_FEAT)
        feat_pl = self._planes(P, B, N_FEAT)
        P.keep.append(self._levels)
        step.append((lib.wd_tpp_max, (cur.t.data_ptr(), cur.c, B, cur.h, cur.w, cur.c, C.addressof(self._levels), len(TPP_LEVELS),
                                      P.feat.data_ptr(), N_FEAT, *self._hilo(feat_pl), N_FEAT), "relu + temporal_pool"))
        h0 = self._f32(P, B, 2 * 4096)
        self._gemm(step, "phos.0 | phoc.0", [self._src(feat_pl, N_FEAT)], "h0.w", B, 1, bias=self._w["h0.b"], out_f32=h0,
                   out_ld=2 * 4096)
        h0_pl, _, _ = self._relu_planes(P, "phos.1 | phoc.1: relu -> planes", Act(h0, 2 * 4096, 1, 1), 1)
        P.logits = {}
        for j, tag in enumerate(("phos", "phoc")):
            h3 = self._f32(P, B, 4096)
            self._gemm(step, tag + ".3", [self._src(h0_pl, 4096, col_off=4096 * j)], tag + ".3.w", B, 1, bias=self._w[tag + ".3.b"],
                       out_f32=h3, out_ld=4096)
            h3_pl, _, _ = self._relu_planes(P, tag + ".4: relu -> planes", Act(h3, 4096, 1, 1), 1)
            rows = self._rows[tag]
            P.logits[tag] = self._f32(P, B, rows)
            self._gemm(step, tag + ".6", [self._src(h3_pl, 4096)], tag + ".6.w", B, 1, bias=self._w[tag + ".6.b"],
                       out_f32=P.logits[tag], out_ld=rows)
        P.out = self._f32(P, B, N_PHOSC)
        step.append((lib.wd_phosc_finish, (P.logits["phos"].data_ptr(), self._rows["phos"], N_PHOS, P.logits["phoc"].data_ptr(),
                                           self._rows["phoc"], N_PHOC, B, P.out.data_ptr(), N_PHOSC), "relu(phos) | sigmoid(phoc)"))
        self._plans[key] = P
        return P

    @staticmethod
    def plan_bytes(P: Plan) -> int:
        """Device bytes a plan holds on to (activations and operand planes; not the packed weights)."""
        return sum(t.numel() * t.element_size() for t in P.keep + [P.x_in] if isinstance(t, torch.Tensor))

    def run(self, x: torch.Tensor, chunk: int) -> Dict[str, torch.Tensor]:
        self.refresh_weights()
        B, _, H, W = x.shape
        dev = self.device
        out = {"features": torch.empty((B, N_FEAT), dtype=torch.float32, device=dev),
               "phosc": torch.empty((B, N_PHOSC), dtype=torch.float32, device=dev),
               "phos_logits": torch.empty((B, N_PHOS), dtype=torch.float32, device=dev),
               "phoc_logits": torch.empty((B, N_PHOC), dtype=torch.float32, device=dev)}
        st = torch.cuda.current_stream(dev).cuda_stream
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            P = self.plan_forward(nb, H, W)
            P.x_in.copy_(x[b0:b0 + nb], non_blocking=True)
            P.run_step(st)
            out["features"][b0:b0 + nb].copy_(P.feat)
            out["phosc"][b0:b0 + nb].copy_(P.out)
            out["phos_logits"][b0:b0 + nb].copy_(P.logits["phos"][:, :N_PHOS])
            out["phoc_logits"][b0:b0 + nb].copy_(P.logits["phoc"][:, :N_PHOC])
        return out


class WordVerifier:
    """Does an image say the word it was asked to say?  ``net``: a ``PHOSCnet`` on the GPU; ``alphabet_csv``: the reference's
    shape-count table (``ResPhoSCNetZSL/modules/utils/Alphabet.csv``); ``size``: the (height, width) the recogniser was trained
    at (``datasets.py:91`` resizes every image to 250 x 50); ``bgr``: flip the channel order while resizing (a recogniser trained
    on ``cv2.imread`` images sees BGR).  Lexicon tables are uploaded once and kept per lexicon."""

    TABLES = 8  # lexicon tables kept (least recently used evicted)

    def __init__(self, net: PHOSCnet, alphabet_csv: str, version: str = "eng", size: Tuple[int, int] = (50, 250), bgr: bool = False):
        from . import phosc as PH
        if not isinstance(net, PHOSCnet):
            raise TypeError(f"net must be a PHOSCnet, got {type(net).__name__}")
        if version not in PH.BIGRAMS:
            raise ValueError(f"version must be one of {sorted(PH.BIGRAMS)}, got {version!r}")
        if len(size) != 2 or min(int(s) for s in size) < 4:
            raise ValueError(f"size must be (height, width), each at least 4, got {size!r}")
        self.net, self.version, self.size, self.bgr = net, version, (int(size[0]), int(size[1])), bool(bgr)
        self.index, self.table = PH.load_alphabet(alphabet_csv)
        self._PH = PH
        self._tables: "collections.OrderedDict[tuple, tuple]" = collections.OrderedDict()

    @property
    def device(self) -> torch.device:
        return next(self.net.parameters()).device

    # ---- images -------------------------------------------------------------------------------------------------------
    def prepare(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 (0..255) or float (0..1) images, [B, 3, H, W] or [B, H, W, 3], any size -> float32 [B, 3, *size] on the
        recogniser's device, resized there by ``wd_resize_bilinear`` (and channel-flipped where ``bgr``)."""
        x = torch.as_tensor(images)
        if x.dim() != 4 or (x.shape[1] != 3 and x.shape[3] != 3):
            raise ValueError(f"images must be [B, 3, H, W] or [B, H, W, 3], got {tuple(x.shape)}")
        if x.dtype != torch.uint8 and not x.is_floating_point():
            raise ValueError(f"images must be uint8 or floating point, got {x.dtype}")
        dev = self.device
        if dev.type != "cuda":
            raise N.NativeError("worddiffusion_amd runs on an MI355X only: move the PHOSCnet to cuda (there is no CPU / eager fallback)")
        x = x.to(dev)
        if x.shape[1] != 3:
            x = x.permute(0, 3, 1, 2)
        x = (x.float() / 255.0 if x.dtype == torch.uint8 else x.float()).contiguous()
        B, _, hs, ws = x.shape
        h, w = self.size
        if (hs, ws) == (h, w) and not self.bgr:
            return x
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        N.check(N.lib().wd_resize_bilinear(x.data_ptr(), ws, B, 3, hs, ws, out.data_ptr(), w, h, w, int(self.bgr), st),
                "wd_resize_bilinear")
        return out

    # ---- lexicons -----------------------------------------------------------------------------------------------------
    def _lexicon(self, words: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(fp32 table [V][772]: the PHOSC vector of every word in a 16-byte row pitch, fp32 row norms [V] from fp64)."""
        key = tuple(words)
        if key in self._tables:
            self._tables.move_to_end(key)
            return self._tables[key]
        if not key or not all(isinstance(wd, str) and wd for wd in key):
            raise ValueError("a lexicon is a non-empty sequence of non-empty words")
        vec = self._PH.phosc_batch(list(key), self.index, self.table, self.version).double()
        if vec.shape[1] != N_PHOSC:
            raise ValueError(f"the PHOSC vector of this alphabet has {vec.shape[1]} entries, the recogniser predicts {N_PHOSC}")
        ld = (N_PHOSC + 3) // 4 * 4
        tab = torch.zeros((len(key), ld), dtype=torch.float32)
        tab[:, :N_PHOSC] = vec.float()
        entry = (tab.to(self.device), vec.norm(dim=1).float().to(self.device))
        self._tables[key] = entry
        while len(self._tables) > self.TABLES:
            self._tables.popitem(last=False)
        return entry

    def _score(self, pred: torch.Tensor, words: Sequence[str], target: Optional[torch.Tensor], want_best: bool):
        tab, norm = self._lexicon(words)
        B, V, dev = pred.shape[0], tab.shape[0], pred.device
        scores = torch.empty((B, V), dtype=torch.float32, device=dev)
        bi = torch.empty((B,), dtype=torch.int32, device=dev) if want_best else None
        bs = torch.empty((B,), dtype=torch.float32, device=dev) if want_best else None
        ts = torch.empty((B,), dtype=torch.float32, device=dev) if target is not None else None
        st = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        N.check(N.lib().wd_phosc_score(pred.data_ptr(), pred.stride(0), B, N_PHOSC, tab.data_ptr(), tab.stride(0), norm.data_ptr(), V,
                                       scores.data_ptr(), V, ptr(bi), ptr(bs), ptr(target), ptr(ts), None, st), "wd_phosc_score")
        return scores, bi, bs, ts

    def _words(self, images, words) -> List[str]:
        words = [words] * len(images) if isinstance(words, str) else list(words)
        if len(words) != len(images):
            raise ValueError(f"{len(images)} images but {len(words)} words")
        return words

    # ---- the public operations ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def score(self, images, words) -> torch.Tensor:
        """fp32 [B]: the cosine of every image's predicted PHOSC against its own word's PHOSC vector."""
        words = self._words(images, words)
        pred = self.net.phosc(self.prepare(images))
        uniq = sorted(set(words))
        target = torch.tensor([uniq.index(wd) for wd in words], dtype=torch.int32, device=pred.device)
        return self._score(pred, uniq, target, False)[3]

    @torch.no_grad()
    def recognise(self, images, lexicon: Sequence[str]):
        """(words, scores fp32 [B], indices int32 [B]): the first best match of every image in ``lexicon``."""
        pred = self.net.phosc(self.prepare(images))
        lexicon = list(lexicon)
        _, bi, bs, _ = self._score(pred, lexicon, None, True)
        return [lexicon[i] for i in bi.tolist()], bs, bi

    @torch.no_grad()
    def verify(self, images, words, min_score: Optional[float] = None, lexicon: Optional[Sequence[str]] = None):
        """One pass of the recogniser for everything the driver logs: (scores fp32 [B] against each image's own word, the best
        word of ``lexicon`` per image or None without one, accepted bool [B]).  A sample is accepted when its score is at least
        ``min_score`` (where given) and, where a lexicon is given, its word is the lexicon's first best match (a word outside
        the lexicon never is); with neither, every sample is accepted."""
        words = self._words(images, words)
        pred = self.net.phosc(self.prepare(images))
        uniq = sorted(set(words))
        target = torch.tensor([uniq.index(wd) for wd in words], dtype=torch.int32, device=pred.device)
        scores = self._score(pred, uniq, target, False)[3]
        ok = torch.ones((len(words),), dtype=torch.bool, device=pred.device)
        if min_score is not None:
            ok &= scores >= float(min_score)
        best = None
        if lexicon is not None:
            lexicon = list(lexicon)
            where = {wd: i for i, wd in reversed(list(enumerate(lexicon)))}  # (the first occurrence of a repeated word)
            want = torch.tensor([where.get(wd, -1) for wd in words], dtype=torch.int32, device=pred.device)
            bi = self._score(pred, lexicon, None, True)[1]
            ok &= bi == want
            best = [lexicon[i] for i in bi.tolist()]
        return scores, best, ok

    @torch.no_grad()
    def check(self, images, words, min_score: Optional[float] = None, lexicon: Optional[Sequence[str]] = None) -> torch.Tensor:
        """bool [B]: ``verify``'s verdict; needs ``min_score``, a lexicon, or both."""
        if min_score is None and lexicon is None:
            raise ValueError("check needs min_score, a lexicon, or both")
        return self.verify(images, words, min_score, lexicon)[2]

"""Time the PHOSCnet recogniser on the GPU and write profiles/phoscnet_time.json (recorded, not gated):

  * ms per 64 images at 50 x 250, and from 64 x 256 through ``WordVerifier.prepare`` (the resize) - device events around REPS
    calls after two warm-up calls;
  * the per-launch table of one plan replay (``wd_prof_*`` classes: time and launches per class);
  * achieved GB/s of each new streaming kernel, launched back to back on the buffers of the plan: the bytes are counted from the
    shapes (what the kernel must read and write once);
  * ``--eager`` (a run of its own, after the plain one): the same network in eager torch-ROCm fp32 on the same GPU
    (``tests/_phoscnet_ref.py`` layout, plain ``F.conv2d`` / ``F.linear``), added to the same file.

Environment: B (64), CHUNK (the class default), REPS (5)."""
import ctypes as C
import json
import os
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _phoscnet_ref as R  # noqa: E402
from worddiffusion_amd import PHOSCnet, WordVerifier  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

B = int(os.environ.get("B", "64"))
REPS = int(os.environ.get("REPS", "5"))
dev = "cuda:0"


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def eager(sd, x):
    h = x
    for j, k in enumerate(R.CONV_KEYS):
        if j:
            h = torch.relu(h)
        if k in R.POOL_BEFORE:
            h = F.max_pool2d(h, (2, 2), stride=2)
        h = F.conv2d(h, sd[f"conv.{k}.weight"], sd[f"conv.{k}.bias"], padding=1)
    feat = R.tpp_torch(torch.relu(h))
    out = []
    for head in ("phos", "phoc"):
        y = feat
        for k in (0, 3, 6):
            y = F.linear(torch.relu(y) if k else y, sd[f"{head}.{k}.weight"], sd[f"{head}.{k}.bias"])
        out.append(torch.relu(y) if head == "phos" else torch.sigmoid(y))
    return torch.cat(out, 1)


def main():
    assert torch.cuda.is_available(), "phoscnet_time.py measures on the MI355X only"
    sd = R.golden_state_dict()
    net = PHOSCnet()
    net.load_state_dict(sd)
    net = net.to(dev)
    if "CHUNK" in os.environ:
        net.chunk = int(os.environ["CHUNK"])
    lib, st = N.lib(), torch.cuda.current_stream().cuda_stream
    res = dict(batch=B, chunk=net.chunk, reps=REPS, device=torch.cuda.get_device_name(0))
    x = torch.rand(B, 3, 50, 250, device=dev)
    res["ms_per_batch_50x250"] = timed(lambda: net.phosc(x), REPS)
    with tempfile.TemporaryDirectory() as tmp:
        ver = WordVerifier(net, R.write_alphabet_csv(os.path.join(ROOT, "tests", "golden"), os.path.join(tmp, "Alphabet.csv")))
    big = torch.rand(B, 3, 64, 256, device=dev)
    res["ms_per_batch_from_64x256_with_resize"] = timed(lambda: net.phosc(ver.prepare(big)), REPS)
    eng = net.engine
    res["plan_bytes_by_batch"] = {str(k[1]): eng.plan_bytes(P) for k, P in eng._plans.items()}
    # ---- one plan replay by kernel class
    P = eng.plan_forward(min(B, net.chunk), 50, 250)
    nb = P.x_in.shape[0]
    P.run_step(st)
    torch.cuda.synchronize()
    ms, cnt, fl = (C.c_double * N.NCLASS)(), (C.c_int64 * N.NCLASS)(), (C.c_double * N.NCLASS)()
    lib.wd_prof_enable(1)
    P.run_step(st)
    lib.wd_prof_collect_flops(ms, cnt, fl)
    lib.wd_prof_enable(0)
    res["plan_replay"] = dict(batch=nb, launches=len(P.step), ops=[what for _, _, what in P.step],
                              classes={name: dict(ms=ms[i], launches=cnt[i], tflops=(fl[i] / (ms[i] * 1e-3) / 1e12 if ms[i] > 0 and fl[i] else None))
                                       for i, name in enumerate(N.CLASS_NAMES) if cnt[i]})
    # ---- the streaming kernels alone, back to back, bytes from the shapes
    stream = {}

    def rate(name, nbytes, fn, reps=50):
        t = timed(fn, reps)
        stream[name] = dict(us=t * 1e3, bytes=nbytes, gb_per_s=nbytes / (t * 1e-3) / 1e9)

    def relu_pool(h, w, c, pool):
        src = torch.randn(nb * h * w, c, device=dev)
        ho, wo = (h // 2, w // 2) if pool == 2 else (h, w)
        pl = torch.empty(2, nb * ho * wo, c, dtype=torch.bfloat16, device=dev)
        rate(f"wd_relu_pool_planes {h}x{w}x{c} pool {pool}", nb * (h * w * c * 4 + ho * wo * c * 4),
             lambda: N.check(lib.wd_relu_pool_planes(src.data_ptr(), c, nb, h, w, c, pool, pl[0].data_ptr(), pl[1].data_ptr(), c, st), "relu"))

    relu_pool(50, 250, 64, 1)
    relu_pool(50, 250, 64, 2)
    relu_pool(25, 125, 128, 2)
    relu_pool(12, 62, 512, 1)
    src = torch.randn(nb * 12 * 62, 512, device=dev)
    feat, fpl = torch.empty(nb, 4096, device=dev), torch.empty(2, nb, 4096, dtype=torch.bfloat16, device=dev)
    lv = (C.c_int32 * 3)(1, 2, 5)
    rate("wd_tpp_max 12x62x512 (three passes over the map, one per level)", nb * (3 * 12 * 62 * 512 * 4 + 4096 * 8),
         lambda: N.check(lib.wd_tpp_max(src.data_ptr(), 512, nb, 12, 62, 512, C.addressof(lv), 3, feat.data_ptr(), 4096, fpl[0].data_ptr(),
                                        fpl[1].data_ptr(), 4096, st), "tpp"))
    small = torch.empty(B, 3, 50, 250, device=dev)
    rate("wd_resize_bilinear 64x256 -> 50x250", B * 3 * (64 * 256 + 50 * 250) * 4,
         lambda: N.check(lib.wd_resize_bilinear(big.data_ptr(), 256, B, 3, 64, 256, small.data_ptr(), 250, 50, 250, 0, st), "resize"))
    V = 10000
    table, norm = torch.rand(V, 772, device=dev), torch.ones(V, device=dev)
    pred, scores = torch.rand(B, 772, device=dev), torch.empty(B, V, device=dev)
    bi = torch.empty(B, dtype=torch.int32, device=dev)
    rate(f"wd_phosc_score B {B} x V {V} (table read once per sample: from L2 / MALL after the first)", B * V * 769 * 4 + B * V * 4,
         lambda: N.check(lib.wd_phosc_score(pred.data_ptr(), 772, B, 769, table.data_ptr(), 772, norm.data_ptr(), V, scores.data_ptr(), V,
                                            bi.data_ptr(), None, None, None, None, st), "score"))
    res["streaming_kernels"] = stream
    out = os.path.join(ROOT, "profiles", "phoscnet_time.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "plan_replay"}, indent=1))
    print("classes:", json.dumps(res["plan_replay"]["classes"]))


def main_eager():
    """--eager: the same network in eager torch fp32 on the same GPU (MIOpen convolutions, rocBLAS linears), added to the JSON the
    plain run wrote.  A run of its own: the first call of every convolution shape pays the library's kernel selection."""
    assert torch.cuda.is_available(), "phoscnet_time.py measures on the MI355X only"
    out = os.path.join(ROOT, "profiles", "phoscnet_time.json")
    with open(out) as f:
        res = json.load(f)
    sd = R.golden_state_dict()
    net = PHOSCnet()
    net.load_state_dict(sd)
    net = net.to(dev)
    x = torch.rand(B, 3, 50, 250, device=dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    with torch.no_grad():
        ms = timed(lambda: eager(sd_dev, x), REPS)
        ref = eager(sd_dev, x[:4])
    res["eager_torch_fp32"] = dict(batch=B, reps=REPS, ms_per_batch_50x250=ms, hip_ms_per_batch_50x250=timed(lambda: net.phosc(x), REPS),
                                   max_abs_diff_of_phosc=float((net.phosc(x[:4]) - ref).abs().max()))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["eager_torch_fp32"], indent=1))


if __name__ == "__main__":
    main_eager() if "--eager" in sys.argv[1:] else main()

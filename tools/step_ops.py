"""Per-launch table of one denoising step at the headline shape (B = 64, base UNet): every op of the plan's step list timed on its own
(hipEvent pair around 20 back-to-back launches, after warm passes of the whole step), with the algorithmic rate of the GEMMs.
Launches run eagerly and alone here (warm L2, no neighbours), so their sum differs a little from the graph's step time.
After the table: one line per launch that ends a step (the samplers' updates and the table-driven advance), timed the same way."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
from worddiffusion_amd import _native as N  # noqa: E402

dev = torch.device("cuda:0")
batch = int(os.environ.get("BATCH", "64"))
variant = os.environ.get("VARIANT", "base")  # "phosc": UNetModelPhosc with the 769-int PHOSC vector
model, args = B.build_model(dev, "bf16x3", variant)
run = B.StepRunner(model, args, dev, batch, 0, 0, phosc_len=769 if variant == "phosc" else 0)
P, st = run.P, run.stream.cuda_stream
REP = 20
rows = []
with torch.cuda.stream(run.stream):
    for _ in range(3):
        P.run_step(st)
    run.stream.synchronize()
    for fn, a, what in P.step:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(run.stream)
        for _ in range(REP):
            N.check(fn(*a, st), what)
        e1.record(run.stream)
        run.stream.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / REP
        info = ""
        obj = getattr(a[0], "_obj", None) if a else None
        if isinstance(obj, N.WdGemmArgs):
            gf = 2.0 * obj.m * obj.n * obj.ktot * 1e-9
            info = f"m={obj.m:6d} n={obj.n:5d} k={obj.ktot:5d} {gf:7.2f} GF {gf / us * 1e3:6.1f} TF/s"
        if isinstance(obj, N.WdFfArgs):
            gf = 2.0 * obj.m * (3.0 * obj.inner * obj.c + (obj.c * obj.c if obj.w3_hi else 0)) * 1e-9
            info = f"m={obj.m:6d} c={obj.c:5d} h={obj.inner:5d} {gf:7.2f} GF {gf / us * 1e3:6.1f} TF/s"
        rows.append((what, getattr(fn, "__name__", str(fn)), us, info))
tot = sum(r[2] for r in rows)
for what, name, us, info in rows:
    print(f"{what[:46]:46s} {name[:22]:22s} {us:8.1f} us  {info}")
print(f"{len(rows)} launches, sum {tot:.1f} us")

# the launches that end a step, one line per sampler's update (not part of the plan's step list: Diffusion._ddpm / _ddim / _dpmpp
# issue them), on a 20-step table of the 1000-step schedule, timed the same way
from worddiffusion_amd import Diffusion  # noqa: E402
lib = N.lib()
diff = Diffusion(noise_steps=1000, img_size=(64, 256), args=args)
tau = diff.dpmpp_timesteps(20)
n, npix = P.x_in.shape[0], P.x_in[0].numel()
ca, cb, cs = (t.data_ptr() for t in diff._step_tables(dev))
ddim_tabs = diff._ddim_tables(tau, 0.0, dev)
dpmpp_tabs = diff._dpmpp_tables(tau, 2, dev)
tau_dev = torch.tensor(tau, dtype=torch.int32, device=dev)
x, eps, prev = torch.randn_like(P.x_in), torch.randn_like(P.x_in), torch.randn_like(P.x_in)
k_dev = torch.ones(1, dtype=torch.int32, device=dev)  # step 1: second order, x0_prev is read
t_dev = torch.tensor([tau[1]], dtype=torch.int32, device=dev)
t64 = torch.zeros(n, dtype=torch.int64, device=dev)
ends = [
    ("ddpm update", lambda s: lib.wd_ddpm_step(x.data_ptr(), eps.data_ptr(), n, npix, ca, cb, cs, t_dev.data_ptr(), None, 5, 0, s)),
    ("ddim update (eta 0)", lambda s: lib.wd_ddim_step(x.data_ptr(), eps.data_ptr(), None, 0.0, None, n, npix,
                                                      *(t.data_ptr() for t in ddim_tabs), k_dev.data_ptr(), t_dev.data_ptr(), None, 5, 0, s)),
    ("dpmpp update (order 2)", lambda s: lib.wd_dpmpp_step(x.data_ptr(), eps.data_ptr(), None, 0.0, None, prev.data_ptr(), n, npix,
                                                         *(t.data_ptr() for t in dpmpp_tabs), k_dev.data_ptr(), s)),
    ("advance over tau", lambda s: lib.wd_next_timestep(k_dev.data_ptr(), tau_dev.data_ptr(), len(tau), t_dev.data_ptr(), t64.data_ptr(), n, s)),
]
with torch.cuda.stream(run.stream):
    for what, fn in ends:
        for _ in range(3):
            N.check(fn(st), what)
        k_dev.fill_(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(run.stream)
        for _ in range(REP):
            N.check(fn(st), what)
        e1.record(run.stream)
        run.stream.synchronize()
        print(f"{what[:46]:46s} {'(ends a step)':22s} {e0.elapsed_time(e1) * 1e3 / REP:8.1f} us")

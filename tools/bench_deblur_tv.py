#!/usr/bin/env python3
"""PSGLA + TV deblurring on the fused kernels, measured: 64 chains x 3 x 256 x 256, uniform 9 x 9 blur (l = 4),
TV(10) at the reference's parameters (s = 10/255, lambda = 10, tol = 1e-5), fast mode.

In one process, alternating over --repeats rounds (HIP events, warm-up first), one JSON line per figure:
  (a) fused_deblur_step     the fused deblurring step: stencil + given-Y TV step, hipGraph replay, per step
  (b) generic_deblur_step   the generic path of this build (the data term wrapped in an opaque closure: a Python
                            loop over stencil + Langevin update, TV prox on the band kernel, relax + accumulate)
  (c) fused_inpaint_step    the inpainting fused step at the same shape (hipGraph replay)
  (d) given_y_kernel / inpaint_kernel   the TV kernel alone (launch_main_only) for both fronts
then the algorithmic HBM bytes of (a) from the shapes and their share of 8 TB/s, and the number of steps (of
--stop-steps) in which deepinv's early stop fired: two engines run side by side, one at tol = 0 (it never stops);
a step after which their states differ stopped somewhere, and the never-stopping engine is then re-synchronised.

    python tools/bench_deblur_tv.py [--steps 200] [--repeats 5] [--out profiles/<tag>_deblur_tv.jsonl]
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E


def fused_deblur_bytes_per_step(B, C, H, W, step0, steps, n_inter, nm):
    """Compulsory HBM bytes of one fused deblurring step, averaged over the timed steps.  Stencil: read X 4 and
    the observation 4, write Y 4.  Step (alpha = 1): read X 4 + u2 8 + Y 4 (+ mean 4 + sq 4 unless the block
    restarts), write X 4 + u2 8 + mean 4 + sq 4 (block means at a block end), + the sample 4 every n_inter steps."""
    E = B * C * H * W
    per = nm + 1
    tot = 0.0
    for i in range(step0, step0 + steps):
        b = 12 + (4 + 8 + 4) + (4 + 8 + 8)
        if i % per != 0:
            b += 8
        if i % n_inter == 0:
            b += 4
        tot += b * E
    return tot / steps


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--H", type=int, default=256)
    p.add_argument("--W", type=int, default=256)
    p.add_argument("--steps", type=int, default=200, help="timed fused steps per round (graph replays)")
    p.add_argument("--generic-steps", type=int, default=40, help="steps of one generic-path call")
    p.add_argument("--kernel-launches", type=int, default=100, help="launch_main_only launches per round")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--graph-steps", type=int, default=20)
    p.add_argument("--stop-steps", type=int, default=1000, help="steps of the early-stop count (0: skip)")
    p.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deblur_tv.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    from psgla_for_posterior_sampling_amd import hip_ops as K
    from psgla_for_posterior_sampling_amd import restoration_algorithms as RA
    from psgla_for_posterior_sampling_amd.denoisers import TVDenoiser
    from psgla_for_posterior_sampling_amd.engine import BlurTerm, FusedTvChains
    from psgla_for_posterior_sampling_amd.fidelity import deblurring_problem, inpainting_problem

    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    B, C, H, W = args.batch, 3, args.H, args.W
    xs = torch.empty((B, C, H, W), device=dev)
    for b in range(B):
        xs[b] = torch.rand((C, H, W), generator=torch.Generator(device=dev).manual_seed(1234 + b), device=dev)
    fid, y_blur, init_blur = deblurring_problem(xs, seed_ip=0, l=4, blur_type="uniform")
    ifid, y_inp, init_inp, _, _ = inpainting_problem(xs, seed_ip=0)
    s = 10 / 255.0
    lam, delta = 10.0, s ** 2
    c1 = float((torch.tensor(delta).float() / torch.tensor(lam).float()).item())
    c2 = float((torch.tensor(np.sqrt(2)).float() * torch.tensor(s).float()).item())
    n_inter = nm = 10
    gs = max(2, args.graph_steps)
    gs += gs & 1
    reps = max(1, args.steps // gs)
    steps = reps * gs
    n_iter = 2 + gs + steps * args.repeats + 8
    common = dict(c1=c1, c2=c2, alpha=1.0, ths=float(np.float32(s)), seed=0, n_inter=n_inter, n_inter_mmse=nm)
    blur = BlurTerm(fid.taps_conv, fid.taps_corr, fid.l, fid.sigma2, False)

    def deblur_engine(tol=1e-5, n_iter=n_iter, **kw):
        return FusedTvChains(init_blur.contiguous(), y_blur.contiguous(), None, sigma2=fid.sigma2,
                             tv=K.TvConstants(n_it_max=10, tol=tol), n_iter=n_iter, blur=blur, **common, **kw)

    eng_d = deblur_engine()
    eng_i = FusedTvChains(init_inp.contiguous(), y_inp.contiguous(), ifid.mask_u8, sigma2=ifid.sigma2,
                          tv=K.TvConstants(n_it_max=10), n_iter=n_iter, **common)
    for e in (eng_d, eng_i):
        e.step(2)
        e.capture(gs)
        e.replay(1)
    torch.cuda.synchronize()
    step0 = eng_d.steps_done

    tv_generic = TVDenoiser(n_it_max=10)

    def generic_call():
        with contextlib.redirect_stdout(io.StringIO()):
            RA.psgla(init_blur, lambda v: fid(v), tv_generic, torch.tensor(1.0), torch.tensor(lam), sig_float=s,
                     delta=delta, n_iter=args.generic_steps, n_inter=n_inter, n_inter_mmse=nm, seed=0)

    generic_call()                                          # warm-up: code objects, allocator
    eng_d.launch_main_only(5)
    eng_i.launch_main_only(5)
    torch.cuda.synchronize()

    res = {k: [] for k in ("a", "b", "c", "d_given", "d_inpaint")}
    nk = args.kernel_launches
    for _ in range(args.repeats):
        res["a"].append(timed(lambda: eng_d.replay(reps)) / steps)
        res["b"].append(timed(generic_call) / args.generic_steps)
        res["c"].append(timed(lambda: eng_i.replay(reps)) / steps)
        eng_d.launch_main_only(1)                           # the step's Y (stencil) outside the timed launches
        d = eng_d.desc.__class__.from_buffer_copy(eng_d.desc)
        d.launch_mask = 1
        res["d_given"].append(timed(lambda: [eng_d._launch(d, stencil=False) for _ in range(nk)]) / nk)
        res["d_inpaint"].append(timed(lambda: eng_i.launch_main_only(nk)) / nk)
    eng_d.check_handoff()
    eng_i.check_handoff()

    def stat(v):
        return {"ms_median": round(float(np.median(v)), 5), "ms_min": round(float(np.min(v)), 5),
                "ms_max": round(float(np.max(v)), 5), "ms_all": [round(float(t), 5) for t in v]}

    shape = {"chains": B, "C": C, "H": H, "W": W, "l": 4, "blur": "uniform", "n_tv": 10, "mode": "fast"}
    emit({"what": "fused_deblur_step", "kernel": eng_d.main_kernel, "per": "step (stencil + given-Y TV step)",
          "timing": f"HIP events over {reps} replays of a {gs}-step hipGraph, {args.repeats} rounds", **shape,
          **stat(res["a"])})
    emit({"what": "generic_deblur_step", "per": "step (Python loop: stencil + prox on the band kernel + relax)",
          "timing": f"HIP events over one psgla() call of {args.generic_steps} steps, {args.repeats} rounds",
          **shape, **stat(res["b"])})
    emit({"what": "fused_inpaint_step", "kernel": eng_i.main_kernel, "per": "step", **shape, **stat(res["c"])})
    emit({"what": "given_y_kernel", "kernel": eng_d.main_kernel, "per": f"launch (launch_main_only, {nk} launches)",
          **shape, **stat(res["d_given"])})
    emit({"what": "inpaint_kernel", "kernel": eng_i.main_kernel, "per": f"launch (launch_main_only, {nk} launches)",
          **shape, **stat(res["d_inpaint"])})
    a_ms, b_ms = float(np.median(res["a"])), float(np.median(res["b"]))
    dg, di = float(np.median(res["d_given"])), float(np.median(res["d_inpaint"]))
    emit({"what": "ratios", "generic_over_fused": round(b_ms / a_ms, 3), "given_y_over_inpaint_kernel": round(dg / di, 4),
          "inpaint_kernel_spread_rel": round((max(res["d_inpaint"]) - min(res["d_inpaint"])) / di, 4)})
    nbytes = fused_deblur_bytes_per_step(B, C, H, W, step0, steps, n_inter, nm)
    gbs = nbytes / (a_ms * 1e-3) / 1e9
    emit({"what": "fused_deblur_roofline", "algorithmic_bytes_per_step": int(nbytes),
          "achieved_GBs": round(gbs, 1), "hbm_peak_GBs": HBM_PEAK_GBS, "share_of_peak": round(gbs / HBM_PEAK_GBS, 4),
          "bound": "HBM bandwidth (whole step over the median step time, stencil included)"})

    if args.stop_steps > 0:
        del eng_i
        n = args.stop_steps
        kw = dict(n_iter=n, store_samples=False, store_blocks=False)
        ea, en = deblur_engine(tol=1e-5, **kw), deblur_engine(tol=0.0, **kw)
        stop_steps, stop_chain_steps, first = 0, 0, []
        for i in range(n):
            ea.step(1)
            en.step(1)
            par = (i + 1) & 1
            diff = (ea.x[par] != en.x[par]).flatten(1).any(1) | (ea.u2[par] != en.u2[par]).flatten(1).any(1)
            k = int(diff.sum().item())
            if k:
                stop_steps += 1
                stop_chain_steps += k
                if len(first) < 20:
                    first.append(i)
                for name in ("x", "u2", "mean", "sq"):
                    getattr(en, name)[par].copy_(getattr(ea, name)[par])
        ea.check_handoff()
        emit({"what": "early_stop_count", "steps": n, "tol": 1e-5, "steps_with_a_stop": stop_steps,
              "chain_steps_with_a_stop": stop_chain_steps, "of_chain_steps": n * B, "first_steps": first,
              "method": "state compared after every step with an engine at tol = 0 (re-synchronised after a stop)"})

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""PnP-ULA + TV (MYULA with a TV prior) deblurring on the fused kernels, measured: 64 chains x 3 x 256 x 256, l = 4
uniform blur, TV(10), fast mode, the CLI's default PnP-ULA parameters for --den TV (s = 5, sigma = 1, alpha = 1, lambd
and delta from sampling_images.algorithm_parameters).  The sibling of tools/bench_ula_tv.py (inpainting).

In one process, alternating over --repeats rounds (HIP events, warm-up first), one JSON line per figure:
  (a) fused_ula_deblur_step   engine.FusedUlaTvDeblurChains: per step the stencil (psgla_blur_grad_pitched) and the fused
                              ULA + TV step (psgla_tv_ula_step, data_term 2), hipGraph replay
  (b) ula_chains_step         the same workload through engine.UlaChains (per step: the stand-alone prox on the band
                              kernel + finaliser, psgla_blur_grad, pnpula_prior_update; eager -- a TVDenoiser is not
                              capturable)
  (c) fused_psgla_deblur_step the fused PSGLA deblurring step at the same shape (stencil + step, hipGraph replay,
                              alpha = 1), for context
  (d) roofline                algorithmic HBM bytes of (a) -- stencil: read X, y, write gd; step: read X, x2, u2, gd,
                              mean, sq; write X', x2, u2, mean, sq: about 64 B per element -- and their share of 8 TB/s
  (e) early_stop_count        the number of steps (of --stop-steps) in which deepinv's early stop fired: two engines run
                              side by side, one at tol = 0 (it never stops); a step after which their states differ
                              stopped somewhere, and the never-stopping engine is then re-synchronised.

    python tools/bench_ula_deblur_tv.py [--steps 200] [--repeats 5] [--out profiles/<tag>_ula_deblur_tv.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E


def fused_bytes_per_step(B, C, H, W, step0, steps, n_inter, nm):
    """Compulsory HBM bytes of one [stencil, fused ULA + TV step] pair, averaged over the timed steps: the stencil reads
    X 4 + y 4 and writes gd 4; the step reads X 4 + x2 4 + u2 8 + gd 4 (+ mean 4 + sq 4 unless the block restarts) and
    writes X' 4 + x2 4 + u2 8 + mean 4 + sq 4 (block means at a block end), + the sample 4 every n_inter steps."""
    E = B * C * H * W
    per = nm + 1
    tot = 0.0
    for i in range(step0, step0 + steps):
        b = 12 + (4 + 4 + 8 + 4) + (4 + 4 + 8 + 8)
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
    p.add_argument("--l", type=int, default=4)
    p.add_argument("--steps", type=int, default=200, help="timed fused steps per round (graph replays)")
    p.add_argument("--chains-steps", type=int, default=40, help="UlaChains steps per round")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--graph-steps", type=int, default=20)
    p.add_argument("--stop-steps", type=int, default=1000, help="steps of the early-stop count (0: skip)")
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ula_deblur_tv.py needs a GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    from psgla_for_posterior_sampling_amd import hip_ops as K
    from psgla_for_posterior_sampling_amd.denoisers import DenoiserPrior, TVDenoiser
    from psgla_for_posterior_sampling_amd.engine import BlurTerm, FusedTvChains, FusedUlaTvDeblurChains, UlaChains
    from psgla_for_posterior_sampling_amd.fidelity import deblurring_problem

    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    B, C, H, W = args.batch, 3, args.H, args.W
    xs = torch.empty((B, C, H, W), device=dev)
    for b in range(B):
        xs[b] = torch.rand((C, H, W), generator=torch.Generator(device=dev).manual_seed(1234 + b), device=dev)
    fid, y, init = deblurring_problem(xs, seed_ip=0, l=args.l, blur_type="uniform")
    blur = BlurTerm(fid.taps_conv, fid.taps_corr, fid.l, fid.sigma2, False)
    # sampling_images.algorithm_parameters, --alg pnp_ula --den TV: s = 5, sigma = 1, alpha = 1
    sigma2, alpha, s1 = (1 / 255.0) ** 2, 1.0, 5.0 / 255.0
    s2 = s1 ** 2
    lambd = 0.5 / (2 / sigma2 + alpha / s2)
    delta = 1 / 3 / (1 / sigma2 + 1 / lambd + alpha / s2)
    delta_f = float(torch.tensor(delta, dtype=torch.float32).item())
    lambd_f = float(torch.tensor(lambd, dtype=torch.float32).item())
    s2_f = float(torch.tensor(s2, dtype=torch.float32).item())
    brw = float(torch.sqrt((2 * torch.tensor(delta, dtype=torch.float32)).double()).float().item())
    n_inter = nm = 10
    gs = max(2, args.graph_steps)
    gs += gs & 1
    reps = max(1, args.steps // gs)
    steps = reps * gs
    n_iter = 2 + gs + steps * args.repeats + 8
    ula = dict(delta=delta_f, lambd=lambd_f, brw=brw, c_min=-1.0, c_max=2.0)

    def ula_engine(tol=1e-5, n_iter=n_iter, **kw):
        return FusedUlaTvDeblurChains(init.contiguous(), y.contiguous(), blur, s2=s2_f, alpha=alpha,
                                      ths=float(np.float32(s1)), tv=K.TvConstants(n_it_max=10, tol=tol), seed=0,
                                      n_iter=n_iter, n_inter=n_inter, n_inter_mmse=nm, **ula, **kw)

    eng_u = ula_engine()
    s = 10 / 255.0
    c1 = float((torch.tensor(s ** 2).float() / torch.tensor(10.0).float()).item())
    c2 = float((torch.tensor(np.sqrt(2)).float() * torch.tensor(s).float()).item())
    eng_p = FusedTvChains(init.contiguous(), y.contiguous(), None, c1=c1, c2=c2, sigma2=fid.sigma2, alpha=1.0,
                          ths=float(np.float32(s)), tv=K.TvConstants(n_it_max=10), seed=0, n_iter=n_iter,
                          n_inter=n_inter, n_inter_mmse=nm, blur=blur)
    for e in (eng_u, eng_p):
        e.step(2)
        e.capture(gs)
        e.replay(1)
    prior = DenoiserPrior(TVDenoiser(n_it_max=10), s1, torch.tensor(alpha, device=dev),
                          torch.tensor(s2, dtype=torch.float32, device=dev))
    cs = args.chains_steps
    eng_c = UlaChains(init.contiguous(), fid, prior, seed=0, n_iter=cs * (args.repeats + 1) + 2, n_inter=n_inter,
                      n_inter_mmse=nm, **ula)
    eng_c.step(cs)                                          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    step0 = eng_u.steps_done

    res = {k: [] for k in ("a", "b", "c")}
    for _ in range(args.repeats):
        res["a"].append(timed(lambda: eng_u.replay(reps)) / steps)
        res["b"].append(timed(lambda: eng_c.step(cs)) / cs)
        res["c"].append(timed(lambda: eng_p.replay(reps)) / steps)
    for e in (eng_u, eng_p):
        e.check_handoff()

    def stat(v):
        return {"ms_median": round(float(np.median(v)), 5), "ms_min": round(float(np.min(v)), 5),
                "ms_max": round(float(np.max(v)), 5), "ms_all": [round(float(t), 5) for t in v]}

    shape = {"chains": B, "C": C, "H": H, "W": W, "l": args.l, "blur": "uniform", "n_tv": 10, "mode": "fast", "s": 5,
             "sigma": 1, "alpha": alpha, "lambd": lambd, "delta": delta}
    emit({"what": "fused_ula_deblur_step", "kernel": eng_u.main_kernel, "per": "step (stencil + fused step)",
          "timing": f"HIP events over {reps} replays of a {gs}-step hipGraph, {args.repeats} rounds", **shape,
          **stat(res["a"])})
    emit({"what": "ula_chains_step",
          "per": "step (prox on the band kernel + finaliser, psgla_blur_grad, pnpula_prior_update; eager)",
          "timing": f"HIP events over {cs} UlaChains steps, {args.repeats} rounds", **shape, **stat(res["b"])})
    emit({"what": "fused_psgla_deblur_step", "kernel": eng_p.main_kernel, "per": "step (stencil + fused step, alpha = 1)",
          **shape, **stat(res["c"])})
    a_ms, b_ms, c_ms = (float(np.median(res[k])) for k in ("a", "b", "c"))
    emit({"what": "ratios", "ula_chains_over_fused_ula": round(b_ms / a_ms, 3),
          "fused_ula_over_fused_psgla_deblur": round(a_ms / c_ms, 4)})
    nbytes = fused_bytes_per_step(B, C, H, W, step0, steps, n_inter, nm)
    gbs = nbytes / (a_ms * 1e-3) / 1e9
    emit({"what": "fused_ula_deblur_roofline", "algorithmic_bytes_per_step": int(nbytes),
          "bytes_per_element": round(nbytes / (B * C * H * W), 2), "achieved_GBs": round(gbs, 1),
          "hbm_peak_GBs": HBM_PEAK_GBS, "share_of_peak": round(gbs / HBM_PEAK_GBS, 4),
          "bound": "HBM bandwidth (algorithmic bytes of both launches over the median step time)"})

    if args.stop_steps > 0:
        del eng_p, eng_c
        n = args.stop_steps
        kw = dict(n_iter=n, store_samples=False, store_blocks=False)
        ea, en = ula_engine(tol=1e-5, **kw), ula_engine(tol=0.0, **kw)
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
                for name in ("x", "x2", "u2", "mean", "sq"):
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

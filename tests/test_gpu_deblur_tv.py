"""PSGLA + TV deblurring on the fused stream / tile / band kernels (PsglaTvStep.data_term 1: the stencil kernel
writes each step's Y, the fused step runs from it) against the CPU oracle, bit for bit in exact mode.

The oracle's data term is ``oracle.blur_grad_tap_order`` -- the restatement the stencil's exact mode equals bit for
bit (torch's conv2d closure is only matched to a tolerance)."""
import os

import numpy as np
import pytest
import torch

from oracle import psgla_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 10 / 255.0
S2 = float(np.float32((1 / 255.0) ** 2))


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from psgla_for_posterior_sampling_amd import _native as N
    N.lib()
    yield


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _taps(l, bt):
    h_ = orc.blur_kernel(l, bt).astype(np.float32)
    return np.flip(h_).copy(), h_                      # hconv, hcorr


def _problem(H, W, l, bt, xseed=5, seed_ip=1):
    x = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(xseed))
    _, y, init = orc.deblurring_problem(x, seed_ip=seed_ip, l=l, blur_type=bt)
    hconv, hcorr = _taps(l, bt)

    def dg(X):
        return torch.from_numpy(orc.blur_grad_tap_order(X.numpy(), y.numpy(), hconv, hcorr, l, S2))
    return dg, y, init, hconv, hcorr


def _engine(prob, B, l, *, n_iter, chain0=0, exact=True, alpha=1.0, variant="auto", stream_wgs=0, n_inter=5,
            n_inter_mmse=4, tol=1e-5, n_tv=10, seed=3):
    from psgla_for_posterior_sampling_amd.engine import BlurTerm, FusedTvChains
    from psgla_for_posterior_sampling_amd import hip_ops as K
    dg, y, init, hconv, hcorr = prob
    c1, c2 = orc.psgla_coefficients(S ** 2, 10.0, S)
    return FusedTvChains(init.expand(B, -1, -1, -1).contiguous().to(DEV), y.to(DEV), None, c1=c1, c2=c2, sigma2=S2,
                         alpha=alpha, ths=float(np.float32(S)), tv=K.TvConstants(n_it_max=n_tv, tol=tol), seed=seed,
                         n_iter=n_iter, n_inter=n_inter, n_inter_mmse=n_inter_mmse, chain0=chain0, exact=exact,
                         kernel_variant=variant, stream_wgs=stream_wgs, blur=BlurTerm(hconv, hcorr, l, S2, exact))


class _RecordingTV(orc.TVDenoiser):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.its = []

    def forward(self, y, ths):
        out = super().forward(y, ths)
        self.its.append(self.last_n_it)
        return out


_ORACLE = {}


def _oracle(key, prob, chain, *, n_iter, alpha=1.0, n_inter=5, n_inter_mmse=4, tol=1e-5, n_tv=10, seed=3):
    """One CPU chain, computed once per (case, chain) and shared by the tests of that case."""
    k = (key, chain, n_iter, alpha, n_inter, n_inter_mmse, tol, n_tv, seed)
    if k not in _ORACLE:
        dg, y, init = prob[:3]
        tv = _RecordingTV(n_it_max=n_tv, tol=tol)
        Xl, Ml, M2l = orc.psgla(init, dg, tv, torch.tensor(alpha), torch.tensor(10.0), sig_float=S, delta=S ** 2,
                                n_iter=n_iter, n_inter=n_inter, n_inter_mmse=n_inter_mmse, seed=seed, chain=chain)
        _ORACLE[k] = (np.stack([t.numpy() for t in Xl]), np.stack([t.numpy() for t in Ml]),
                      np.stack([t.numpy() for t in M2l]), tv.x2.numpy()[0], tv.u2.numpy()[0], list(tv.its))
    return _ORACLE[k]


def _assert_engine_equals_oracle(eng, key, prob, B, chain0, alpha=1.0, **kw):
    torch.cuda.synchronize()
    eng.check_handoff()
    sm = eng.samples().cpu().numpy()
    bm, bm2 = (t.cpu().numpy() for t in eng.blocks())
    u2 = eng.u2_state.cpu().numpy()
    x2 = eng.x2_state.cpu().numpy()
    its = []
    for b in range(B):
        Xs, Ms, M2s, ox2, ou2, it = _oracle(key, prob, chain0 + b, alpha=alpha, **kw)
        its.append(it)
        np.testing.assert_array_equal(sm[:, b], Xs)
        np.testing.assert_array_equal(bm[:, b], Ms)
        np.testing.assert_array_equal(bm2[:, b], M2s)
        np.testing.assert_array_equal(u2[b], ou2)
        if alpha != 1.0:
            np.testing.assert_array_equal(x2[b], ox2)
    return its


# ------------------------------------------------------------------ 1. exact vs oracle, stream kernel
STREAM_CASES = [
    # B, H, W, l, blur, alpha, stream_wgs
    (3, 48, 64, 4, "gaussian", 1.0, 0), (3, 48, 64, 4, "gaussian", 1.0, -1),
    (3, 48, 64, 4, "gaussian", 1.0, 7),            # cuts inside planes, ranges spanning planes
    (2, 23, 29, 4, "uniform", 1.0, 0),             # W % 4 != 0: padded pitch in the stencil and the step
    (2, 21, 33, 4, "uniform", 0.6, 0),             # alpha != 1: x2 state, relaxation
    (1, 17, 321, 4, "uniform", 1.0, 0),            # half-wave windows, castle's width
    (2, 11, 483, 2, "uniform", 1.0, 0),            # column segments
]


@pytest.mark.parametrize("B,H,W,l,bt,alpha,wgs", STREAM_CASES)
def test_stream_exact_vs_oracle(B, H, W, l, bt, alpha, wgs):
    n = 15
    prob = _problem(H, W, l, bt)
    eng = _engine(prob, B, l, n_iter=n, chain0=10, alpha=alpha, variant="stream", stream_wgs=wgs)
    assert eng.main_kernel == "tv_stream_kernel"
    eng.run(n, graph_steps=0)
    _assert_engine_equals_oracle(eng, (H, W, l, bt), prob, B, 10, alpha=alpha, n_iter=n)


# ------------------------------------------------------------------ 2. exact vs oracle, tile kernel
@pytest.mark.parametrize("B,H,W,l,alpha", [(2, 100, 64, 4, 1.0),     # 48-row tiles, several bands with halo cuts
                                           (1, 70, 52, 4, 0.6),      # 32-row tiles
                                           (1, 40, 301, 4, 1.0)])    # GEN: padded pitch and column segments
def test_tile_exact_vs_oracle(B, H, W, l, alpha):
    n = 12
    prob = _problem(H, W, l, "uniform")
    eng = _engine(prob, B, l, n_iter=n, chain0=10, alpha=alpha, variant="tile")
    assert eng.main_kernel == "tv_tile_kernel"
    eng.run(n, graph_steps=0)
    _assert_engine_equals_oracle(eng, (H, W, l, "uniform"), prob, B, 10, alpha=alpha, n_iter=n)


# ------------------------------------------------------------------ 3. exact vs oracle, band kernel
@pytest.mark.parametrize("B,variant,n_tv", [(2, "band", 10), (1, "auto", 14)])
def test_band_exact_vs_oracle(B, variant, n_tv):
    n = 12
    prob = _problem(40, 52, 4, "uniform")
    eng = _engine(prob, B, 4, n_iter=n, chain0=10, variant=variant, n_tv=n_tv)
    if variant == "band":
        assert eng.main_kernel == "tv_main_kernel"
    eng.run(n, graph_steps=0)
    _assert_engine_equals_oracle(eng, (40, 52, 4, "uniform"), prob, B, 10, n_iter=n, n_tv=n_tv)


# ------------------------------------------------------------------ 4. early stop: the finaliser's serial recompute
@pytest.mark.parametrize("variant,wgs", [("stream", 0), ("stream", -1), ("tile", 0)])
def test_early_stop_serial_recompute_exact_vs_oracle(variant, wgs):
    """tol = 2e-3: on the CPU oracle the inner-iteration counts are [3,10,10,10,8,6,6,6,4,4,4,4] (chain 0) and
    [3,10,10,10,8,6,6,4,4,4,4,4] (chain 1): full steps, stops at several depths, one step where the chains differ.
    With a given Y there is no parallel redo: the step's finaliser re-reads Y and recomputes the stopped chains."""
    B, H, W, l, n, tol = 2, 40, 52, 4, 12, 2e-3
    prob = _problem(H, W, l, "uniform", xseed=7, seed_ip=2)
    kw = dict(n_iter=n, n_inter=3, n_inter_mmse=2, tol=tol, seed=4)
    eng = _engine(prob, B, l, variant=variant, stream_wgs=wgs, **kw)
    assert eng.desc.redo is None and eng.desc.data_term == 1
    assert eng.main_kernel == ("tv_stream_kernel" if variant == "stream" else "tv_tile_kernel")
    eng.run(n, graph_steps=0)
    its = _assert_engine_equals_oracle(eng, ("es", H, W, l), prob, B, 0, **kw)
    print("inner iterations per step:", its)
    flat = [k for it in its for k in it]
    assert min(flat) < 10, "the test needs the early stop to fire"
    assert max(flat) == 10, "the test needs a step that runs every inner iteration"
    assert its[0] != its[1], "the test needs a step where the two chains stop at different depths"
    eng.check_handoff()


# ------------------------------------------------------------------ 5. graph replay and batching
@pytest.mark.parametrize("W", [64, 29])
@pytest.mark.parametrize("eager_first", [1, 2])
def test_chains_independent_of_batching_and_graph_parity(W, eager_first):
    """Chain k depends only on (seed, global chain id): B = 4 eager vs B = 2 from chain0 = 2 replayed from a graph of
    [stencil, step] pairs captured at an odd (eager_first = 1) or even (2) step -- the stencil picks its input by the
    device step's parity.  Fast mode, bit-identical."""
    n, H = 40, 48
    prob = _problem(H, W, 4, "uniform")
    e4 = _engine(prob, 4, 4, n_iter=n, chain0=0, exact=False)
    e4.run(n, graph_steps=0)
    e2 = _engine(prob, 2, 4, n_iter=n, chain0=2, exact=False)
    e2.step(eager_first)
    e2.run(n - eager_first, graph_steps=10)
    assert e2.graph is not None and e2.steps_done == n
    torch.cuda.synchronize()
    assert torch.equal(e4.X[2:], e2.X)
    b4, q4 = e4.blocks()
    b2, q2 = e2.blocks()
    assert torch.equal(b4[:, 2:], b2) and torch.equal(q4[:, 2:], q2)
    assert torch.equal(e4.samples()[:, 2:], e2.samples())


# ------------------------------------------------------------------ 6. psgla_blur_langevin
def _stencil_case(B, H, W, l=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, H, W), generator=g)
    A, _ = orc.blur_operators(l=l, blur_type="gaussian")
    y = A(x) + torch.normal(torch.zeros_like(x), (1 / 255.0) * torch.ones_like(x), generator=g)
    xs = (x + 0.05 * torch.randn(x.shape, generator=g)).contiguous()
    hconv, hcorr = _taps(l, "gaussian")
    return xs.to(DEV), y.to(DEV), hconv, hcorr


@pytest.mark.parametrize("B,H,W", [(2, 40, 52), (1, 37, 29)])
@pytest.mark.parametrize("exact", [True, False])
def test_blur_langevin_contiguous_equals_blur_grad_path(B, H, W, exact):
    from psgla_for_posterior_sampling_amd import hip_ops as K
    X, y, hconv, hcorr = _stencil_case(B, H, W)
    want = K.blur_langevin(X, y, hconv, hcorr, 4, S2, 1e-4, 0.05, seed=9, chain0=3, step=17, exact=exact)
    got = K.blur_langevin_pitched(X, X, y, hconv, hcorr, 4, S2, 1e-4, 0.05, 9, 3, 17, torch.empty_like(X), W,
                                  exact=exact)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("exact", [True, False])
def test_blur_langevin_padded_pitch_equals_contiguous(exact):
    """ld = 32 on 37 x 29: the image columns equal the contiguous run; the padding columns are not written."""
    from psgla_for_posterior_sampling_amd import hip_ops as K
    W, ld = 29, 32
    X, y, hconv, hcorr = _stencil_case(1, 37, W)
    want = K.blur_langevin(X, y, hconv, hcorr, 4, S2, 1e-4, 0.05, seed=9, chain0=3, step=17, exact=exact)
    # padding columns of the inputs hold a value that would show in the output if it were read
    Xp = torch.full((1, 3, 37, ld), 1e3, device=DEV)
    yp = torch.full((1, 3, 37, ld), -1e3, device=DEV)
    Xp[..., :W] = X
    yp[..., :W] = y
    out = torch.full((1, 3, 37, ld), 7.0, device=DEV)
    K.blur_langevin_pitched(Xp, Xp, yp, hconv, hcorr, 4, S2, 1e-4, 0.05, 9, 3, 17, out, W, exact=exact)
    torch.cuda.synchronize()
    assert torch.equal(out[..., :W], want)
    assert bool((out[..., W:] == 7.0).all())


def test_blur_langevin_selects_its_input_by_step_parity():
    from psgla_for_posterior_sampling_amd import hip_ops as K
    Xe, y, hconv, hcorr = _stencil_case(2, 40, 52)
    Xo = (Xe * 0.5 + 0.1).contiguous()
    for step, Xsel in ((6, Xe), (7, Xo)):
        d_step = torch.full((1,), step, dtype=torch.int64, device=DEV)
        want = K.blur_langevin(Xsel, y, hconv, hcorr, 4, S2, 1e-4, 0.05, seed=9, chain0=3, step=step, exact=True)
        got = K.blur_langevin_pitched(Xe, Xo, y, hconv, hcorr, 4, S2, 1e-4, 0.05, 9, 3, 0, torch.empty_like(Xe), 52,
                                      exact=True, d_step=d_step)
        torch.cuda.synchronize()
        assert torch.equal(got, want), step


# ------------------------------------------------------------------ 7. given-Y front against the inpainting front
@pytest.mark.parametrize("variant", ["stream", "tile"])
def test_given_y_front_equals_inpainting_front(variant):
    """GPU vs GPU, both exact: feeding the new front the inpainting step's own Y = langevin_update(X,
    inpaint_grad(X)) must reproduce the inpainting fused step (oracle-pinned by test_gpu_parity) bit for bit --
    state, TV dual, live accumulators, samples and block means, over several steps."""
    from psgla_for_posterior_sampling_amd.engine import BlurTerm, FusedTvChains
    from psgla_for_posterior_sampling_amd import hip_ops as K
    B, H, W, n = 2, 48, 64, 6
    x = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(5))
    _, y, init, mask2d = orc.inpainting_problem(x, seed_ip=1)
    c1, c2 = orc.psgla_coefficients(S ** 2, 10.0, S)
    init_b = init.expand(B, -1, -1, -1).contiguous().to(DEV)
    yd, mk = y.to(DEV), mask2d.to(torch.uint8).to(DEV)
    common = dict(c1=c1, c2=c2, sigma2=S2, alpha=1.0, ths=float(np.float32(S)), tv=K.TvConstants(n_it_max=10), seed=3,
                  n_iter=n, n_inter=2, n_inter_mmse=2, chain0=10, exact=True, kernel_variant=variant)
    ei = FusedTvChains(init_b, yd, mk, **common)
    hconv, hcorr = _taps(4, "uniform")
    eg = FusedTvChains(init_b, yd, None, blur=BlurTerm(hconv, hcorr, 4, S2, True), **common)
    assert eg.main_kernel == ei.main_kernel
    for i in range(n):
        Xi = eg.X.contiguous()
        K.langevin_update(Xi, K.inpaint_grad(Xi, yd, mk, S2), c1, c2, 3, 10, i, out=eg.Ybuf)
        eg._launch(eg.desc, stencil=False)          # the fused step alone, from the Y just written
        eg.steps_done += 1
        ei.step(1)
        torch.cuda.synchronize()
        assert torch.equal(eg.X, ei.X), i
        assert torch.equal(eg.u2_state, ei.u2_state), i
        par = (i + 1) & 1
        if (i + 1) % 3:                              # inside a block: the live accumulators
            assert torch.equal(eg.mean[par], ei.mean[par]) and torch.equal(eg.sq[par], ei.sq[par]), i
    assert torch.equal(eg.samples(), ei.samples())
    for a, b in zip(eg.blocks(), ei.blocks()):
        assert a.shape[0] == 2 and torch.equal(a, b)


# ------------------------------------------------------------------ 8. psgla() end to end
def test_psgla_typed_call_takes_the_fused_engine_and_equals_the_generic_path(monkeypatch):
    from psgla_for_posterior_sampling_amd import restoration_algorithms as RA
    from psgla_for_posterior_sampling_amd.denoisers import TVDenoiser
    from psgla_for_posterior_sampling_amd.engine import FusedTvChains
    from psgla_for_posterior_sampling_amd.fidelity import deblurring_problem
    x = torch.rand((1, 3, 40, 52), generator=torch.Generator().manual_seed(5)).to(DEV)
    dg, y, init = deblurring_problem(x, seed_ip=1, l=4, blur_type="uniform")
    dg.exact = True
    init2 = init.expand(2, -1, -1, -1).contiguous()
    calls = {"n": 0}
    launch = FusedTvChains._launch

    def counted(self, *a, **k):
        calls["n"] += 1
        return launch(self, *a, **k)
    monkeypatch.setattr(FusedTvChains, "_launch", counted)
    kw = dict(sig_float=S, delta=S ** 2, n_iter=20, n_inter=5, n_inter_mmse=4, seed=3, chain0=10)
    tv_f, tv_g = TVDenoiser(n_it_max=10, exact=True), TVDenoiser(n_it_max=10, exact=True)
    for call in range(2):                            # the second call warm-starts from the denoiser's state
        before = calls["n"]
        out_f = RA.psgla(init2, dg, tv_f, torch.tensor(1.0), torch.tensor(10.0), **kw)
        assert calls["n"] - before == 20, "the typed call must run on FusedTvChains"
        before = calls["n"]
        out_g = RA.psgla(init2, lambda v: dg(v), tv_g, torch.tensor(1.0), torch.tensor(10.0), **kw)
        assert calls["n"] == before, "an opaque closure stays on the generic branch"
        torch.cuda.synchronize()
        for lf, lg in zip(out_f, out_g):
            assert len(lf) == len(lg) > 0
            for a, b in zip(lf, lg):
                assert torch.equal(a, b), call
        assert torch.equal(tv_f.x2, tv_g.x2) and torch.equal(tv_f.u2, tv_g.u2)


# ------------------------------------------------------------------ 9. fast vs exact
@pytest.mark.parametrize("variant", ["stream", "tile"])
def test_fast_vs_exact(variant):
    """The project's standing contract of the fused step (test_fused_full_size_fast_vs_exact): block means within
    1e-5 relative of exact mode, X within 1e-4, everything finite -- here with the stencil's fast (separable) mode on
    top of the fast TV kernels."""
    B, H, W, n = 4, 96, 128, 12
    prob = _problem(H, W, 4, "uniform")
    outs = []
    for exact in (True, False):
        eng = _engine(prob, B, 4, n_iter=n, exact=exact, variant=variant, n_inter=10, n_inter_mmse=10)
        eng.run(n, graph_steps=0)
        torch.cuda.synchronize()
        outs.append((eng.X.clone().cpu().numpy(), eng.blocks()[0].clone().cpu().numpy()))
    (xe, be), (xf, bf) = outs
    assert np.isfinite(xe).all() and np.isfinite(xf).all() and np.isfinite(bf).all()
    rb, rx = rel(bf, be), rel(xf, xe)
    print(f"deblur fast vs exact ({variant}): block means rel {rb:.3g}, X rel {rx:.3g}")
    assert rb <= 1e-5
    assert rx <= 1e-4


# ------------------------------------------------------------------ 10. CLI
def test_cli_deblurring_tv_batched_equals_sequential(tmp_path):
    """--Pb deblurring --den TV inherits the fused path through psgla(): two 40 x 52 images as one batch of 2 and
    one by one give the same per-image MMSE, bit for bit (fast mode; chains are keyed by their global id).
    N = 1000: the CLI's n_inter = int(N / 1000) must be >= 1 (a smaller N raises, as in the reference);
    --tv_restart: a sequential run otherwise warm-starts TV from the previous image."""
    from PIL import Image
    from psgla_for_posterior_sampling_amd import engine, sampling_images as SI
    d = tmp_path / "datasets" / "synth"
    os.makedirs(d)
    rng = np.random.default_rng(5)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (40, 52, 3)).astype(np.uint8)).save(str(d / f"{i:04d}.png"))
    seen = []
    init = engine.FusedTvChains.__init__

    def spy(self, *a, **k):
        seen.append(k.get("blur") is not None)
        return init(self, *a, **k)
    engine.FusedTvChains.__init__ = spy
    try:
        runs = {}
        for bs in (2, 1):
            argv = ["--alg", "psgla", "--den", "TV", "--Pb", "deblurring", "--dataset_name", "synth", "--N", "1000",
                    "--datasets_root", str(tmp_path / "datasets"), "--results_root", str(tmp_path / f"r{bs}"),
                    "--no_plots", "--tv_restart", "--batch_size", str(bs)]
            runs[bs] = SI.main(argv)
    finally:
        engine.FusedTvChains.__init__ = init
    assert seen == [True, True, True], "the CLI's deblurring + TV runs must take the fused engine"
    assert len(runs[1]) == len(runs[2]) == 2
    for a, b in zip(runs[2], runs[1]):
        assert np.isfinite(a["PSNR_MMSE"]) and a["PSNR_MMSE"] > a["PSNR_y"]
        np.testing.assert_array_equal(np.asarray(a["MMSE"]), np.asarray(b["MMSE"]))

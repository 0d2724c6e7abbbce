"""The fused PnP-ULA + TV step with the deblurring data term (psgla_tv_ula_step with tv.data_term 2: the stencil
kernel writes the data gradient of the step's input, the fused step reads it) on the row stream and the band kernel
against the CPU oracle -- ``oracle.pnpula`` with ``oracle.TVDenoiser``, one oracle run per chain, ``data_grad`` =
``oracle.blur_grad_tap_order`` (the restatement the stencil's exact mode equals bit for bit) --, bit for bit in exact
mode: samples, block means of X and X^2, final X, x2 and u2.  ULA parameters as tests/test_gpu_ula_tv.py."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import psgla_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S1 = 5 / 255.0                                     # s = 5, sigma = 1: the CLI's PnP-ULA defaults for --den TV
SIG2 = float(np.float32((1 / 255.0) ** 2))
FAST_REL_BOUND = 1e-5                              # the project's standing bound for the fast steps (test_gpu_ula_tv.py)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32).item())


def _params(alpha):
    """lambd and delta of algorithm_parameters (sampling_images.py:118-119), as the fp32 tensors the CLI passes."""
    sigma2, s2 = (1 / 255.0) ** 2, S1 ** 2
    lambd = 0.5 / (2 / sigma2 + alpha / s2)
    delta = 1 / 3 / (1 / sigma2 + 1 / lambd + alpha / s2)
    return torch.tensor(delta, dtype=torch.float32), torch.tensor(lambd, dtype=torch.float32)


@pytest.fixture(scope="module", autouse=True)
def _native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from psgla_for_posterior_sampling_amd import _native as N
    N.lib()
    yield


def _taps(l, bt):
    h_ = orc.blur_kernel(l, bt).astype(np.float32)
    return np.flip(h_).copy(), h_                      # hconv, hcorr


_PROBLEMS = {}


def _problem(H, W, l, bt, xseed=5, seed_ip=1, smooth=False, bands=False):
    """(data_grad, y, init, hconv, hcorr) on the CPU.  smooth: the 5 x 5 box-smoothed image of
    test_gpu_ula_tv._problem(smooth=True).  bands: rows 0-9 of the image are 0 and rows 10-19 are 1, so that the
    blurred observation is noise around 0 and around 1 inside them (a blur of iid pixels stays near 0.5)."""
    k = (H, W, l, bt, xseed, seed_ip, smooth, bands)
    if k not in _PROBLEMS:
        x = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(xseed))
        if smooth:                                 # box average 5 x 5, replicate padding
            x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="replicate"), 5, stride=1)
        if bands:
            x[:, :, :10] = 0.0
            x[:, :, 10:20] = 1.0
        _, y, init = orc.deblurring_problem(x, seed_ip=seed_ip, l=l, blur_type=bt)
        hconv, hcorr = _taps(l, bt)

        def dg(X, y=y, hconv=hconv, hcorr=hcorr):
            return torch.from_numpy(orc.blur_grad_tap_order(X.numpy(), y.numpy(), hconv, hcorr, l, SIG2))
        _PROBLEMS[k] = (dg, y, init, hconv, hcorr)
    return _PROBLEMS[k]


def _engine(prob, B, l, *, n_iter, chain0=0, exact=True, alpha=1.0, variant="auto", stream_wgs=0, n_inter=5,
            n_inter_mmse=4, tol=1e-5, n_tv=10, seed=3, c_min=-1.0, c_max=2.0, cls=None, blur_exact=None):
    from psgla_for_posterior_sampling_amd import hip_ops as K
    from psgla_for_posterior_sampling_amd.engine import BlurTerm, FusedUlaTvDeblurChains
    _, y, init1, hconv, hcorr = prob
    delta, lambd = _params(alpha)
    brw = float(orc.sqrt_rn(2 * delta).item())
    cls = FusedUlaTvDeblurChains if cls is None else cls
    bterm = BlurTerm(hconv, hcorr, l, SIG2, exact if blur_exact is None else blur_exact)
    return cls(init1.expand(B, -1, -1, -1).contiguous().to(DEV), y.to(DEV), bterm, delta=float(delta),
               lambd=float(lambd), brw=brw, c_min=c_min, c_max=c_max, s2=_f32(S1 ** 2), alpha=_f32(alpha),
               ths=float(np.float32(S1)), tv=K.TvConstants(n_it_max=n_tv, tol=tol), seed=seed, n_iter=n_iter,
               n_inter=n_inter, n_inter_mmse=n_inter_mmse, chain0=chain0, exact=exact, kernel_variant=variant,
               stream_wgs=stream_wgs)


class _RecordingTV(orc.TVDenoiser):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.its = []

    def forward(self, y, ths):
        out = super().forward(y, ths)
        self.its.append(self.last_n_it)
        return out


_ORACLE = {}


def _oracle(key, prob, chain, *, n_iter, alpha=1.0, n_inter=5, n_inter_mmse=4, tol=1e-5, n_tv=10, seed=3, c_min=-1.0,
            c_max=2.0):
    """One CPU chain, computed once per (case, chain) and shared by the tests of that case: (samples, block means of
    X, of X^2, x2, u2, inner iterations per step, final X).  The oracle stores every step (n_inter = 1), so the
    samples are every n_inter-th of them and the final X is the last."""
    k = (key, chain, n_iter, alpha, n_inter_mmse, tol, n_tv, seed, c_min, c_max)
    if k not in _ORACLE:
        dg, y, init = prob[:3]
        tv = _RecordingTV(n_it_max=n_tv, tol=tol)
        alphat, s2t = torch.tensor(alpha, dtype=torch.float32), torch.tensor(S1 ** 2, dtype=torch.float32)
        delta, lambd = _params(alpha)
        Xl, Ml, M2l = orc.pnpula(init, dg, lambda x: alphat * (tv.forward(x, S1) - x) / s2t, delta, lambd,
                                 n_iter=n_iter, n_inter=1, n_inter_mmse=n_inter_mmse, seed=seed, c_min=c_min,
                                 c_max=c_max, chain=chain)
        _ORACLE[k] = (np.stack([t.numpy() for t in Xl]), np.stack([t.numpy() for t in Ml]),
                      np.stack([t.numpy() for t in M2l]), tv.x2.numpy()[0], tv.u2.numpy()[0], list(tv.its))
    Xall, Ms, M2s, x2, u2, its = _ORACLE[k]
    return Xall[::n_inter], Ms, M2s, x2, u2, its, Xall[-1]


def _assert_engine_equals_oracle(eng, key, prob, B, chain0, **kw):
    torch.cuda.synchronize()
    eng.check_handoff()
    sm = eng.samples().cpu().numpy()
    bm, bm2 = (t.cpu().numpy() for t in eng.blocks())
    u2 = eng.u2_state.cpu().numpy()
    x2 = eng.x2_state.cpu().numpy()
    X = eng.X.cpu().numpy()
    its = []
    for b in range(B):
        Xs, Ms, M2s, ox2, ou2, it, Xfin = _oracle(key, prob, chain0 + b, **kw)
        its.append(it)
        np.testing.assert_array_equal(sm[:, b], Xs)
        np.testing.assert_array_equal(bm[:, b], Ms)
        np.testing.assert_array_equal(bm2[:, b], M2s)
        np.testing.assert_array_equal(u2[b], ou2)
        np.testing.assert_array_equal(x2[b], ox2)
        np.testing.assert_array_equal(X[b], Xfin)
    return its


# ------------------------------------------------------------------ 1. exact vs oracle, row stream
STREAM_CASES = [
    # B, H, W, l, blur, stream_wgs
    (3, 48, 64, 4, "gaussian", 0), (3, 48, 64, 4, "gaussian", -1),
    (3, 48, 64, 4, "gaussian", 7),                 # cuts inside planes, ranges spanning planes
    (2, 23, 29, 4, "uniform", 0),                  # W % 4 != 0: padded pitch in the stencil and the step
    (1, 17, 321, 4, "uniform", 0),                 # half-wave windows, castle's width
    (2, 11, 483, 2, "uniform", 0),                 # column segments
]


@pytest.mark.parametrize("B,H,W,l,bt,wgs", STREAM_CASES)
def test_stream_exact_vs_oracle(B, H, W, l, bt, wgs):
    n = 15
    prob = _problem(H, W, l, bt)
    eng = _engine(prob, B, l, n_iter=n, chain0=10, variant="stream", stream_wgs=wgs)
    assert eng.main_kernel == "tv_stream_kernel"
    assert eng.ldw == (W + 3) // 4 * 4
    eng.run(n, graph_steps=0)
    _assert_engine_equals_oracle(eng, (H, W, l, bt), prob, B, 10, n_iter=n)


def test_stream_exact_vs_oracle_projection_and_alpha():
    """Prior alpha = 0.6 and c_min, c_max = 0, 1 at 2 x 21 x 33, l = 4 uniform.  The observation must leave [0, 1] for
    the projection term (X - proj) / lambd to be non-zero; a 9 x 9 blur of iid uniform pixels stays near 0.5, so the
    image of this case carries a band of zeros and a band of ones (_problem(bands=True)), inside which the observation
    is the noise around 0 and around 1."""
    B, H, W, l, n = 2, 21, 33, 4, 15
    prob = _problem(H, W, l, "uniform", bands=True)
    kw = dict(n_iter=n, alpha=0.6, c_min=0.0, c_max=1.0)
    y = prob[1].numpy()
    assert (y < 0).any() and (y > 1).any()
    eng = _engine(prob, B, l, chain0=10, variant="stream", **kw)
    assert eng.main_kernel == "tv_stream_kernel"
    eng.run(n, graph_steps=0)
    _assert_engine_equals_oracle(eng, (H, W, l, "bands"), prob, B, 10, **kw)


# ------------------------------------------------------------------ 1b. exact vs oracle, band kernel
@pytest.mark.parametrize("B,H,W,variant,n_tv", [(2, 40, 52, "band", 10), (1, 40, 52, "auto", 14),
                                                (2, 23, 29, "auto", 14)])      # unpadded scalar path
def test_band_exact_vs_oracle(B, H, W, variant, n_tv):
    n, l = 15, 4
    prob = _problem(H, W, l, "uniform")
    eng = _engine(prob, B, l, n_iter=n, chain0=10, variant=variant, n_tv=n_tv)
    assert eng.main_kernel == "tv_main_kernel"
    assert eng.ldw == W                            # the band kernel runs unpadded
    eng.run(n, graph_steps=0)
    _assert_engine_equals_oracle(eng, (H, W, l, "uniform"), prob, B, 10, n_iter=n, n_tv=n_tv)


# ------------------------------------------------------------------ 2. early stop: the finaliser's serial recompute
# inner-iteration counts of the CPU oracle for this input (tol 1e-4, 30 steps, seed 4), chains 0 and 1
ES_COUNTS = ([10] * 21 + [8, 6, 4, 6, 4, 4, 6, 4, 4], [10] * 21 + [8, 6, 6, 4, 4, 6, 4, 4, 4])


@pytest.mark.parametrize("variant,wgs", [("stream", 0), ("stream", -1), ("band", 0)])
def test_early_stop_serial_recompute_exact_vs_oracle(variant, wgs):
    """deepinv's early stop per chain: full steps, stops at several depths and three steps where the two chains stop
    at different depths.  With a given gradient there is no parallel redo: the step's finaliser re-reads the gradient
    and recomputes the stopped chains."""
    B, H, W, l, n, tol = 2, 40, 52, 2, 30, 1e-4
    prob = _problem(H, W, l, "uniform", xseed=7, seed_ip=2, smooth=True)
    kw = dict(n_iter=n, n_inter=3, n_inter_mmse=2, tol=tol, seed=4)
    eng = _engine(prob, B, l, variant=variant, stream_wgs=wgs, **kw)
    assert eng.desc.tv.redo is None and eng.desc.tv.data_term == 2
    assert eng.main_kernel == ("tv_stream_kernel" if variant == "stream" else "tv_main_kernel")
    eng.run(n, graph_steps=0)
    its = _assert_engine_equals_oracle(eng, ("es", H, W, l), prob, B, 0, **kw)
    print("inner iterations per step:", its)
    assert (its[0], its[1]) == ES_COUNTS
    eng.check_handoff()


# ------------------------------------------------------------------ 3. the given-gradient front == the inpainting front
def _state(eng):
    torch.cuda.synchronize()
    b1, b2 = eng.blocks()
    return [t.clone() for t in (eng.samples(), b1, b2, eng.X, eng.x2_state, eng.u2_state)]


@pytest.mark.parametrize("variant", ["stream", "band"])
def test_given_gradient_front_equals_the_inpainting_front(variant):
    """On an inpainting problem: FRONT_ULA (the data term computed in the kernel) against a data_term 2 descriptor whose
    gradient buffer holds psgla_inpaint_grad of the step's input -- all state bit-identical in exact mode."""
    from psgla_for_posterior_sampling_amd import hip_ops as K
    from psgla_for_posterior_sampling_amd.engine import FusedUlaTvChains, FusedUlaTvDeblurChains
    B, H, W, n = 2, 24, 40, 8
    x = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(5))
    _, y, init, mask2d = orc.inpainting_problem(x, seed_ip=1, prop=0.5, sigma=1.0)
    yd, md = y.to(DEV), mask2d.to(torch.uint8).to(DEV)
    delta, lambd = _params(1.0)
    brw = float(orc.sqrt_rn(2 * delta).item())
    x0 = init.expand(B, -1, -1, -1).contiguous().to(DEV)
    kw = dict(delta=float(delta), lambd=float(lambd), brw=brw, c_min=-1.0, c_max=2.0, s2=_f32(S1 ** 2), alpha=1.0,
              ths=float(np.float32(S1)), tv=K.TvConstants(n_it_max=10, tol=1e-5), seed=3, n_iter=n, n_inter=3,
              n_inter_mmse=2, chain0=10, exact=True, kernel_variant=variant)
    ref = FusedUlaTvChains(x0, yd, md, sigma2=SIG2, **kw)

    class InpaintGradient(FusedUlaTvDeblurChains):
        def _launch(self, desc, stencil=True):
            K.inpaint_grad(self.x[self.steps_done & 1], yd, md, SIG2, out=self.Ybuf)     # ldw == W here
            super()._launch(desc, stencil=False)

    hconv, hcorr = _taps(1, "uniform")             # never used: the override writes the gradient
    from psgla_for_posterior_sampling_amd.engine import BlurTerm
    giv = InpaintGradient(x0, yd, BlurTerm(hconv, hcorr, 1, SIG2, True), **kw)
    want = "tv_stream_kernel" if variant == "stream" else "tv_main_kernel"
    assert ref.main_kernel == want and giv.main_kernel == want
    assert giv.ldw == W and giv.desc.tv.data_term == 2 and ref.desc.tv.data_term == 0
    ref.run(n, graph_steps=0)
    giv.run(n, graph_steps=0)
    for u, v in zip(_state(giv), _state(ref)):
        assert torch.equal(u, v)


# ------------------------------------------------------------------ 4. the stencil entry point
@pytest.mark.parametrize("B,H,W", [(2, 40, 52), (1, 37, 29)])
@pytest.mark.parametrize("exact", [True, False])
def test_blur_grad_pitched(B, H, W, exact):
    from psgla_for_posterior_sampling_amd import hip_ops as K
    l = 4
    hconv, hcorr = _taps(l, "gaussian")
    gen = torch.Generator().manual_seed(11)
    Xa, Xb, y = (torch.rand((B, 3, H, W), generator=gen).to(DEV) for _ in range(3))
    ga = K.blur_grad(Xa, y, hconv, hcorr, l, SIG2, exact=exact)
    gb = K.blur_grad(Xb, y, hconv, hcorr, l, SIG2, exact=exact)
    assert not torch.equal(ga, gb)
    # contiguous: bit-identical to psgla_blur_grad; the input is selected by the step's parity
    out = torch.empty_like(Xa)
    assert torch.equal(K.blur_grad_pitched(Xa, Xa, y, hconv, hcorr, l, SIG2, 0, out, W, exact=exact), ga)
    assert torch.equal(K.blur_grad_pitched(Xa, Xb, y, hconv, hcorr, l, SIG2, 0, out, W, exact=exact), ga)
    assert torch.equal(K.blur_grad_pitched(Xa, Xb, y, hconv, hcorr, l, SIG2, 1, out, W, exact=exact), gb)
    d_step = torch.tensor([6], dtype=torch.int64, device=DEV)
    assert torch.equal(K.blur_grad_pitched(Xa, Xb, y, hconv, hcorr, l, SIG2, 1, out, W, exact=exact, d_step=d_step), gb)
    assert torch.equal(K.blur_grad_pitched(Xa, Xb, y, hconv, hcorr, l, SIG2, 0, out, W, exact=exact, d_step=d_step), ga)
    # padded pitch: the image columns are the contiguous run's, the padding columns are left as they were
    ld = W // 4 * 4 + 4

    def pad(t, fill):
        p = torch.full(t.shape[:-1] + (ld,), fill, dtype=t.dtype, device=t.device)
        p[..., :W] = t
        return p
    outp = torch.full((B, 3, H, ld), 7.0, device=DEV)
    K.blur_grad_pitched(pad(Xa, 3.0), pad(Xb, -3.0), pad(y, 5.0), hconv, hcorr, l, SIG2, 1, outp, W, exact=exact)
    torch.cuda.synchronize()
    assert torch.equal(outp[..., :W], gb)
    assert bool((outp[..., W:] == 7.0).all())


# ------------------------------------------------------------------ 5. batching and replay
@pytest.mark.parametrize("W", [64, 29])
def test_batch_equals_single_chains_and_replay_equals_eager(W):
    B, H, n, l = 3, 24, 13, 4
    prob = _problem(H, W, l, "uniform")
    kw = dict(n_iter=n, n_inter=3, n_inter_mmse=2)
    eager = _engine(prob, B, l, chain0=10, **kw)
    assert eager.main_kernel == "tv_stream_kernel"
    eager.run(n, graph_steps=0)
    ref = _state(eager)
    for b in range(B):                               # a batch of 3 == each chain alone with its chain0
        one = _engine(prob, 1, l, chain0=10 + b, **kw)
        one.run(n, graph_steps=0)
        for j, (u, v) in enumerate(zip(_state(one), ref)):
            # samples / block means: (slot, chain, C, H, W); X, x2, u2: (chain, ...)
            assert torch.equal(u[:, 0], v[:, b]) if j < 3 else torch.equal(u[0], v[b])
    replay = _engine(prob, B, l, chain0=10, **kw)    # graph replay (3 graphs of 4 steps + 1 eager step) == eager
    replay.run(n, graph_steps=4)
    assert replay.graph is not None and replay.graph_steps == 4
    for u, v in zip(_state(replay), ref):
        assert torch.equal(u, v)
    odd = _engine(prob, B, l, chain0=10, **kw)       # capture after an odd number of eager steps
    odd.step(3)
    odd.run(n - 3, graph_steps=4)
    assert odd.graph is not None
    for u, v in zip(_state(odd), ref):
        assert torch.equal(u, v)


# ------------------------------------------------------------------ 6. the public call
def _spy(monkeypatch):
    from psgla_for_posterior_sampling_amd import restoration_algorithms as RA
    made = []

    class Spy(RA.FusedUlaTvDeblurChains):
        def __init__(self, *a, **kw):
            made.append(1)
            super().__init__(*a, **kw)
    monkeypatch.setattr(RA, "FusedUlaTvDeblurChains", Spy)
    return made


def _public_problem(H=24, W=40, l=2):
    from psgla_for_posterior_sampling_amd.fidelity import deblurring_problem
    x = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(1)).to(DEV)
    dg, _, init = deblurring_problem(x, seed_ip=0, l=l)
    return dg, init


def test_pnpula_takes_the_fused_engine_and_equals_the_generic_path(monkeypatch):
    from psgla_for_posterior_sampling_amd import restoration_algorithms as RA
    from psgla_for_posterior_sampling_amd.denoisers import DenoiserPrior, TVDenoiser
    made = _spy(monkeypatch)
    dg, init = _public_problem()
    delta, lambd = _params(1.0)
    alphat, s2t = torch.tensor(1.0, device=DEV), torch.tensor(S1 ** 2, dtype=torch.float32, device=DEV)
    tv_a, tv_b = TVDenoiser(n_it_max=10, exact=True), TVDenoiser(n_it_max=10, exact=True)
    pa, pb = DenoiserPrior(tv_a, S1, alphat, s2t), DenoiserPrior(tv_b, S1, alphat, s2t)
    kw = dict(n_iter=20, n_inter=3, n_inter_mmse=3, seed=9)
    for rnd in range(2):                             # the second call continues warm from the denoiser's state
        a = RA.pnpula(init, dg, pa, delta, lambd, graph_steps=4, **kw)
        assert len(made) == rnd + 1
        b = RA.pnpula(init, lambda x: dg(x), lambda x: pb(x), delta, lambd, **kw)   # the generic closure path
        assert len(made) == rnd + 1
        for la, lb in zip(a, b):
            assert len(la) == len(lb) > 0
            for u, v in zip(la, lb):
                assert torch.equal(u, v)
        assert torch.equal(tv_a.x2, tv_b.x2) and torch.equal(tv_a.u2, tv_b.u2)
        assert tv_a.restart is False and tv_b.restart is False


def test_pnpula_long_prox_keeps_its_path(monkeypatch):
    from psgla_for_posterior_sampling_amd import restoration_algorithms as RA
    from psgla_for_posterior_sampling_amd.denoisers import DenoiserPrior, TVDenoiser
    made = _spy(monkeypatch)
    dg, init = _public_problem()
    delta, lambd = _params(1.0)
    alphat, s2t = torch.tensor(1.0, device=DEV), torch.tensor(S1 ** 2, dtype=torch.float32, device=DEV)
    out = RA.pnpula(init, dg, DenoiserPrior(TVDenoiser(n_it_max=30, exact=True), S1, alphat, s2t), delta, lambd,
                    n_iter=10, n_inter=3, n_inter_mmse=3, seed=9)
    assert not made and len(out[0]) == 4 and torch.isfinite(torch.stack(out[0])).all()


def test_save_images_online_keeps_the_fused_engine(tmp_path, monkeypatch):
    from psgla_for_posterior_sampling_amd import restoration_algorithms as RA
    from psgla_for_posterior_sampling_amd.denoisers import DenoiserPrior, TVDenoiser
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_dnn import _check_snapshots
    made = _spy(monkeypatch)
    B, n = 3, 40
    dg, init1 = _public_problem(24, 40)
    init = init1.repeat(B, 1, 1, 1).contiguous()
    delta, lambd = _params(1.0)
    alphat, s2t = torch.tensor(1.0, device=DEV), torch.tensor(S1 ** 2, dtype=torch.float32, device=DEV)
    mk = lambda: DenoiserPrior(TVDenoiser(n_it_max=10, exact=True), S1, alphat, s2t)   # noqa: E731
    kw = dict(n_iter=n, n_inter=3, n_inter_mmse=4, seed=4, graph_steps=4)
    a = RA.pnpula(init, dg, mk(), delta, lambd, **kw)
    b = RA.pnpula(init, dg, mk(), delta, lambd, path=str(tmp_path), save_images_online=True, name="nm", **kw)
    assert len(made) == 2
    for la, lb in zip(a, b):
        assert len(la) == len(lb) > 0
        for u, v in zip(la, lb):
            assert torch.equal(u, v)
    i_last = _check_snapshots(str(tmp_path), "nm", n, b, ("c_min", "c_max", "lambda", "delta"), False, B)
    d = torch.load(str(tmp_path) + "/nm_sampling.pth", weights_only=True)
    assert len(d["Samples"]) == i_last // 3 + 1
    assert len(d["Mmse"]) == (i_last + 1) // 5
    assert d["n_iter"] == n


# ------------------------------------------------------------------ 7. fast vs the exact CPU oracle
def _maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("variant", ["stream", "band"])
def test_fast_vs_oracle(variant):
    """Fast mode (the separable stencil; fmas, host-formed reciprocals, rsq in the TV dual) against the exact CPU
    oracle after 200 steps, 2 x 48 x 64, l = 4 uniform: the maximum difference of the final X and of the block means
    of X, relative to the largest magnitude of the oracle's.  The bound is the project's standing 1e-5 (measured, the
    same on both kernels: 1.91e-6 for the final X, 2.12e-6 for the block means)."""
    B, H, W, l, n = 2, 48, 64, 4, 200
    prob = _problem(H, W, l, "uniform")
    kw = dict(n_iter=n, n_inter=50, n_inter_mmse=49)
    eng = _engine(prob, B, l, exact=False, variant=variant, **kw)
    assert eng.main_kernel == ("tv_stream_kernel" if variant == "stream" else "tv_main_kernel")
    eng.run(n, graph_steps=0)
    torch.cuda.synchronize()
    eng.check_handoff()
    X = eng.X.cpu().numpy()
    bm = eng.blocks()[0].cpu().numpy()
    worst = 0.0
    for b in range(B):
        o = _oracle(("fast", H, W, l), prob, b, **kw)
        dx = _maxrel(X[b], o[6])
        dm = _maxrel(bm[:, b], o[1])
        print(f"fast ULA+TV deblurring {variant} chain {b}: max rel diff final X = {dx:.3g}, block means = {dm:.3g}")
        worst = max(worst, dx, dm)
    assert worst <= FAST_REL_BOUND, worst


# ------------------------------------------------------------------ 8. CLI
def test_cli_pnpula_tv_deblurring_batched_equals_sequential(tmp_path, monkeypatch):
    """--alg pnp_ula --den TV --Pb deblurring inherits the fused engine, sequential and --batch_size-batched.  The
    CLI's TV denoiser and stencil run in fast mode: the two runs' MMSE agree within the fast bound."""
    from psgla_for_posterior_sampling_amd import sampling_images as SI
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_cli import _dataset, _records
    made = _spy(monkeypatch)
    droot = _dataset(str(tmp_path), n=2, h=24, w=32)
    common = ["--alg", "pnp_ula", "--den", "TV", "--Pb", "deblurring", "--dataset_name", "synth", "--N", "1000",
              "--datasets_root", droot, "--no_plots", "--tv_restart"]
    recs = SI.main(common + ["--results_root", str(tmp_path / "seq")])
    assert len(recs) == 2 and len(made) == 2
    SI.main(common + ["--results_root", str(tmp_path / "batch"), "--batch_size", "2"])
    assert len(made) == 3
    seq, bat = _records(str(tmp_path / "seq"), 2), _records(str(tmp_path / "batch"), 2)
    for ra, rb in zip(seq, bat):
        assert ra["n_iter"] == 1000 and len(ra["PSNR_sample"]) == 1000
        assert np.isfinite(ra["PSNR_MMSE"]) and ra["PSNR_MMSE"] > ra["PSNR_y"]
        np.testing.assert_array_equal(np.asarray(ra["observation"]), np.asarray(rb["observation"]))
        d = _maxrel(rb["MMSE"], ra["MMSE"])
        print(f"CLI pnp_ula TV deblurring batch vs sequential: max rel diff of MMSE = {d:.3g}")
        assert d <= FAST_REL_BOUND, d

"""CPU-side checks of the fused PnP-ULA + TV step's second data term, "the data gradient is given"
(psgla_tv_ula_step with tv.data_term 2), and of the pitched stencil entry point that writes the gradient,
psgla_blur_grad_pitched: binding, ABI version, the host-side kernel choice and the rejected descriptors.  Nothing is
launched."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "psgla_hip.h")
BAND, STREAM = 0, 1


def test_blur_grad_pitched_is_exported_and_bound_with_the_headers_arity():
    from psgla_for_posterior_sampling_amd import _native as N
    assert "psgla_blur_grad_pitched" in N.EXPORTED_SYMBOLS
    assert hasattr(N.lib(), "psgla_blur_grad_pitched")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bpsgla_blur_grad_pitched\s*\(([^)]*)\)\s*;", src)
    assert m
    params = [p for p in m.group(1).split(",") if p.strip()]
    assert len(params) == len(N._SIGNATURES["psgla_blur_grad_pitched"][1]) == 18
    from psgla_for_posterior_sampling_amd import hip_ops as K
    assert callable(K.blur_grad_pitched)


def test_abi_version_is_12():
    from psgla_for_posterior_sampling_amd import _native as N
    assert N.ABI_VERSION == 12 == N.lib().psgla_abi_version()
    # symbols and meanings only: the descriptors keep their layouts
    assert [f[0] for f in N.PsglaTvStep._fields_][-1] == "data_term"
    assert [f[0] for f in N.PsglaUlaTvStep._fields_] == ["tv", "delta", "lambd", "brw", "c_min", "c_max", "s2"]


def _kind(B, H, W, ldw=0, n_tv=10, variant=0, data_term=0, redo=False):
    from psgla_for_posterior_sampling_amd import _native as N
    lib = N.lib()
    d = N.PsglaUlaTvStep()
    t = d.tv
    t.B, t.C, t.H, t.W, t.ldw, t.n_tv, t.kernel_variant, t.data_term = B, 3, H, W, ldw, n_tv, variant, data_term
    t.x2[0], t.x2[1] = 16, 32              # non-null (the query never dereferences them)
    if redo:
        t.redo = 64
    k = lib.psgla_tv_ula_step_kernel(ctypes.byref(d))
    return k, (lib.psgla_last_error().decode() if k < 0 else "")


# the seven shapes of test_ula_tv_host.test_ula_kernel_dispatch_on_the_host and the kernel each takes
ULA_DISPATCH = [
    (dict(B=64, H=256, W=256), STREAM), (dict(B=8, H=256, W=256), STREAM),
    (dict(B=1, H=481, W=321, ldw=324), STREAM), (dict(B=64, H=256, W=256, n_tv=14), BAND),
    (dict(B=1, H=256, W=256, n_tv=14), BAND), (dict(B=64, H=256, W=256, variant=1), BAND),
    (dict(B=8, H=256, W=256, variant=2), STREAM),
]


def test_given_gradient_takes_the_kernel_of_the_inpainting_term():
    for kw, want in ULA_DISPATCH:
        k0, e0 = _kind(data_term=0, **kw)
        k2, e2 = _kind(data_term=2, **kw)
        assert k0 == want, (kw, k0, e0)
        assert k2 == k0, (kw, k2, e2)


def test_given_gradient_rejects_a_redo_buffer():
    k, err = _kind(64, 256, 256, data_term=2, redo=True)
    assert k == -1 and "redo" in err
    assert _kind(64, 256, 256, data_term=0, redo=True)[0] == STREAM      # the inpainting term keeps its parallel redo


def test_other_data_terms_stay_rejected():
    for dt in (1, 3):
        k, err = _kind(64, 256, 256, data_term=dt)
        assert k == -1 and "data_term" in err, (dt, k, err)


def test_tv_step_keeps_rejecting_a_given_gradient():
    from psgla_for_posterior_sampling_amd import _native as N
    lib = N.lib()
    d = N.PsglaTvStep()
    d.B, d.C, d.H, d.W, d.n_tv, d.data_term = 64, 3, 256, 256, 10, 2
    assert lib.psgla_tv_step_kernel(ctypes.byref(d)) == -1
    assert "data_term" in lib.psgla_last_error().decode()

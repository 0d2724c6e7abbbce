"""CPU-side checks of ABI 12: the fused TV step's "Y is given" data term (PsglaTvStep.data_term) and the pitched
stencil entry point psgla_blur_langevin.  Host-side queries only: nothing is launched."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "psgla_hip.h")


def test_abi_version_is_12():
    from psgla_for_posterior_sampling_amd import _native as N
    assert N.ABI_VERSION == 12 == N.lib().psgla_abi_version()


def test_tv_step_descriptor_has_data_term_last():
    from psgla_for_posterior_sampling_amd import _native as N
    names = [f[0] for f in N.PsglaTvStep._fields_]
    assert "data_term" in names
    # appended: a zero-initialised ABI 11 descriptor keeps its meaning
    assert names[-1] == "data_term" and names[-2] == "redo"
    assert N.PsglaTvStep().data_term == 0


def test_blur_langevin_is_exported_with_the_headers_arity():
    from psgla_for_posterior_sampling_amd import _native as N
    assert "psgla_blur_langevin" in N.EXPORTED_SYMBOLS
    assert hasattr(N.lib(), "psgla_blur_langevin")
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bpsgla_blur_langevin\s*\(([^)]*)\)\s*;", src)
    assert m
    params = [p for p in m.group(1).split(",") if p.strip()]
    assert len(params) == len(N._SIGNATURES["psgla_blur_langevin"][1]) == 22


def _kind(data_term, B, H, W, ldw=0, n_tv=10, variant=0):
    from psgla_for_posterior_sampling_amd import _native as N
    lib = N.lib()
    d = N.PsglaTvStep()
    d.B, d.C, d.H, d.W, d.ldw, d.n_tv, d.kernel_variant = B, 3, H, W, ldw, n_tv, variant
    d.data_term = data_term
    k = lib.psgla_tv_step_kernel(ctypes.byref(d))
    return k, (lib.psgla_last_error().decode() if k < 0 else "")


# the shapes of test_kernel_dispatch_rules_on_the_host and the kernel each takes (0 band, 1 stream, 3 tile)
DISPATCH = [
    (dict(B=64, H=256, W=256), 1), (dict(B=16, H=256, W=256), 3), (dict(B=8, H=256, W=256), 3),
    (dict(B=1, H=481, W=321, ldw=324), 3), (dict(B=8, H=481, W=321, ldw=324), 1),
    (dict(B=1, H=256, W=256, n_tv=14), 3), (dict(B=64, H=256, W=256, n_tv=14), 0),
    (dict(B=64, H=256, W=256, variant=1), 0), (dict(B=8, H=256, W=256, variant=2), 1),
    (dict(B=64, H=256, W=256, variant=4), 3),
]


def test_kernel_choice_does_not_depend_on_the_data_term():
    for kw, want in DISPATCH:
        k0, e0 = _kind(0, **kw)
        k1, e1 = _kind(1, **kw)
        assert k0 == want, (kw, k0, e0)
        assert k1 == k0, (kw, k1, e1)


def test_unknown_data_term_is_rejected():
    k, err = _kind(2, 64, 256, 256)
    assert k == -1 and "data_term" in err
    k, err = _kind(-1, 8, 256, 256)
    assert k == -1 and "data_term" in err

"""CPU-side checks of the fused PnP-ULA + TV step's entry points (psgla_tv_ula_step, psgla_tv_ula_step_kernel, added
to ABI 12 as symbols only): binding, descriptor layout and the host-side kernel choice.  Nothing is launched."""
import ctypes
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "psgla_hip.h")
BAND, STREAM = 0, 1


def test_ula_symbols_are_exported_and_bound_with_the_headers_arity():
    from psgla_for_posterior_sampling_amd import _native as N
    lib = N.lib()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, arity in (("psgla_tv_ula_step", 3), ("psgla_tv_ula_step_kernel", 1)):
        assert name in N.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip()]
        assert len(params) == len(N._SIGNATURES[name][1]) == arity


def test_abi_version_stays_12_and_the_tv_descriptor_is_embedded_unchanged():
    from psgla_for_posterior_sampling_amd import _native as N
    assert N.ABI_VERSION == 12 == N.lib().psgla_abi_version()
    names = [f[0] for f in N.PsglaUlaTvStep._fields_]
    assert names == ["tv", "delta", "lambd", "brw", "c_min", "c_max", "s2"]
    assert N.PsglaUlaTvStep._fields_[0][1] is N.PsglaTvStep
    assert [f[0] for f in N.PsglaTvStep._fields_][-1] == "data_term"


def test_ula_descriptor_layout_matches_c(tmp_path):
    from psgla_for_posterior_sampling_amd import _native as N
    fs = [f[0] for f in N.PsglaUlaTvStep._fields_]
    lines = ['#include "psgla_hip.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void){",
             'printf("size %zu\\n", sizeof(PsglaUlaTvStep));', 'printf("tvsize %zu\\n", sizeof(PsglaTvStep));']
    lines += [f'printf("{f} %zu\\n", offsetof(PsglaUlaTvStep, {f}));' for f in fs]
    lines.append("return 0;}")
    prog = tmp_path / "sz.c"
    prog.write_text("\n".join(lines))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(l.rsplit(" ", 1) for l in out if l)
    assert int(got["size"]) == ctypes.sizeof(N.PsglaUlaTvStep)
    assert int(got["tvsize"]) == ctypes.sizeof(N.PsglaTvStep)
    for f in fs:
        assert int(got[f]) == getattr(N.PsglaUlaTvStep, f).offset, f


def _kind(B, H, W, ldw=0, n_tv=10, variant=0, x2=True, data_term=0):
    from psgla_for_posterior_sampling_amd import _native as N
    lib = N.lib()
    d = N.PsglaUlaTvStep()
    t = d.tv
    t.B, t.C, t.H, t.W, t.ldw, t.n_tv, t.kernel_variant, t.data_term = B, 3, H, W, ldw, n_tv, variant, data_term
    if x2:
        t.x2[0], t.x2[1] = 16, 32          # non-null (the query never dereferences them)
    k = lib.psgla_tv_ula_step_kernel(ctypes.byref(d))
    return k, (lib.psgla_last_error().decode() if k < 0 else "")


def test_ula_kernel_dispatch_on_the_host():
    """No tile kernel yet: shapes psgla_tv_step gives to tiles run on the row stream, or on the band kernel when
    n_tv > 10; psgla_tv_ula_step_kernel never answers 3."""
    assert _kind(64, 256, 256)[0] == STREAM
    assert _kind(8, 256, 256)[0] == STREAM
    assert _kind(1, 481, 321, ldw=324)[0] == STREAM
    assert _kind(64, 256, 256, n_tv=14)[0] == BAND
    assert _kind(1, 256, 256, n_tv=14)[0] == BAND
    assert _kind(64, 256, 256, variant=1)[0] == BAND
    assert _kind(8, 256, 256, variant=2)[0] == STREAM


def test_ula_rejected_descriptors():
    k, err = _kind(64, 256, 256, variant=4)
    assert k == -1 and "tile" in err
    k, err = _kind(1, 481, 321, ldw=324, variant=1)              # the band kernel needs ldw == W
    assert k == -1 and "row pitch" in err
    k, err = _kind(64, 256, 256, x2=False)
    assert k == -1 and "x2" in err
    k, err = _kind(64, 256, 256, data_term=1)
    assert k == -1 and "data_term" in err
    k, err = _kind(64, 256, 256, variant=3)
    assert k == -1 and "kernel_variant" in err

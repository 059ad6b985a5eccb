"""CPU, library cross-compiled: the host-side argument checks of exo_lbfgs_f64 (no launch is reached: the pointers of the
table are no addresses of anything).  That header and binding table agree: tests/test_abi.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from exoplanet_amd import _lib

    return _lib.load()


def test_entry_point_checks_its_arguments_on_the_host(lib):
    n_ptr = 22
    full = (ctypes.c_void_p * n_ptr)(*([8] * n_ptr))          # (8 is no address of anything: a pointer that were followed would fault)
    ok = dict(ptrs=full, n_chain=4, n_param=3, n_hist=8, max_linesearch=20, c1=1e-4, gtol=1e-5, ftol=1e-9, phase=0, stream=None)

    def call(**kw):
        return lib.exo_lbfgs_f64(*{**ok, **kw}.values())

    for bad in (dict(ptrs=None), dict(n_chain=-1), dict(n_param=0), dict(n_param=-2), dict(n_hist=0), dict(n_hist=33),
                dict(max_linesearch=0), dict(phase=2), dict(phase=-1)):
        assert call(**bad) == INVALID, bad
    for k in range(n_ptr):                                     # a null entry, whichever
        gap = (ctypes.c_void_p * n_ptr)(*[None if i == k else 8 for i in range(n_ptr)])
        assert call(ptrs=gap) == INVALID and call(ptrs=gap, phase=1) == INVALID, k
    # no chains: nothing is launched, the table is not looked at; sizes are checked first
    assert call(n_chain=0) == 0 and call(n_chain=0, phase=1) == 0
    assert call(n_chain=0, ptrs=(ctypes.c_void_p * n_ptr)()) == 0
    assert call(n_chain=0, n_hist=33) == INVALID and call(n_chain=0, phase=2) == INVALID and call(n_chain=0, ptrs=None) == INVALID


def test_header_constant_binding_and_abi_number():
    from exoplanet_amd import _lib
    from exoplanet_amd.optimize import MAX_HISTORY

    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    assert int(re.search(r"#define\s+EXO_LBFGS_MAX_HISTORY\s+(\d+)", text).group(1)) == MAX_HISTORY == 32
    assert int(re.search(r"#define\s+EXO_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 21   # (a new entry point, no new number)
    assert len(_lib._SIGNATURES["exo_lbfgs_f64"][1]) == 10
    assert "HOST array of 22 device pointers" in text

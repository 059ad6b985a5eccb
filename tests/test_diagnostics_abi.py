"""CPU, library cross-compiled: the host-side argument checks of the exo_diag_* entry points (no launch is reached: the
pointers are no addresses of anything).  That header and binding table agree: tests/test_abi.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = 1, 3
P8 = 8          # (no address of anything: a pointer that were followed would fault)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry

    entry.build()
    from exoplanet_amd import _lib

    return _lib.load()


def test_workspace_size(lib):
    P, M, L = 3, 66, 37
    n_wave, l_pad = 2, 48
    assert lib.exo_diag_workspace_bytes(P, M, L) == 8 * P * 5 * (M + n_wave * 16 + l_pad + 8)
    assert lib.exo_diag_workspace_bytes(0, M, L) == 0
    for bad in ((-1, M, L), (P, -2, L), (P, M, 1), (P, 65, L), (13108, M, L)):
        assert lib.exo_diag_workspace_bytes(*bad) == -1, bad


def test_entry_points_check_their_arguments_on_the_host(lib):
    P, M, L = 3, 66, 37
    S = M * L
    nbytes = lib.exo_diag_workspace_bytes(P, M, L)
    prepare = dict(x=P8, sorted=P8, sorted_full=P8, n_full=S, n_param=P, n_half=M, n_len=L, folded=P8, sets=P8, moments=P8,
                   stream=None)
    rank = dict(sorted=P8, perm=P8, n_param=P, n_half=M, n_len=L, set=0, sets=P8, stream=None)
    autocov = dict(sets=P8, n_param=P, n_half=M, n_len=L, block=0, done=P8, workspace=P8, workspace_bytes=nbytes, stream=None)
    finish = dict(n_param=P, n_half=M, n_len=L, block=0, moments=None, out=None, done=P8, workspace=P8, workspace_bytes=nbytes,
                  stream=None)
    entries = ((lib.exo_diag_prepare_f64, prepare), (lib.exo_diag_rank_f64, rank), (lib.exo_diag_autocov_f64, autocov),
               (lib.exo_diag_finish_f64, finish))
    sizes = (dict(n_param=-1), dict(n_half=-2), dict(n_half=65), dict(n_len=1), dict(n_len=-5), dict(n_param=13108))
    for fn, ok in entries:
        for bad in sizes:
            assert fn(*{**ok, **bad}.values()) == INVALID, (fn.__name__, bad)
        for key, value in ok.items():
            if value == P8:                                            # a null pointer, whichever
                assert fn(*{**ok, key: None}.values()) == INVALID, (fn.__name__, key)
        # nothing to do: no launch, the pointers are not looked at; sizes are checked first
        empty = {k: (None if v == P8 else v) for k, v in ok.items()}
        assert fn(*{**empty, "n_param": 0}.values()) == 0 and fn(*{**empty, "n_half": 0}.values()) == 0, fn.__name__
        assert fn(*{**empty, "n_param": 0, "n_len": 1}.values()) == INVALID, fn.__name__
    assert lib.exo_diag_prepare_f64(*{**prepare, "n_full": S - 1}.values()) == INVALID
    assert lib.exo_diag_rank_f64(*{**rank, "set": 2}.values()) == INVALID and lib.exo_diag_rank_f64(*{**rank, "set": -1}.values()) == INVALID
    for fn, ok in entries[2:]:
        assert fn(*{**ok, "workspace_bytes": nbytes - 1}.values()) == WORKSPACE, fn.__name__
        assert fn(*{**ok, "block": 3}.values()) == INVALID, fn.__name__        # 37 draws: lag blocks 0, 1, 2
    assert lib.exo_diag_autocov_f64(*{**autocov, "block": -1}.values()) == INVALID
    # the last call: block -1 needs the moments and the output
    assert lib.exo_diag_finish_f64(*{**finish, "block": -1}.values()) == INVALID
    assert lib.exo_diag_finish_f64(*{**finish, "block": -2, "moments": P8, "out": P8}.values()) == INVALID


def test_header_constants_and_binding():
    from exoplanet_amd import _lib, diagnostics, ops

    text = open(os.path.join(ROOT, "include", "exoplanet_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(EXO_DIAG_[A-Z_]+)\s+(\d+)", text))
    assert int(consts["EXO_DIAG_LAG_BLOCK"]) == ops.DIAG_LAG_BLOCK == diagnostics.LAG_BLOCK == 16
    assert int(consts["EXO_DIAG_SETS"]) == ops.DIAG_SETS == 5 and int(consts["EXO_DIAG_MOMENTS"]) == ops.DIAG_MOMENTS
    assert int(consts["EXO_DIAG_OUT"]) == ops.DIAG_OUT == len(ops.DIAG_COLUMNS)
    assert int(re.search(r"#define\s+EXO_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION
    assert [len(_lib._SIGNATURES[k][1]) for k in ("exo_diag_workspace_bytes", "exo_diag_prepare_f64", "exo_diag_rank_f64",
                                                  "exo_diag_autocov_f64", "exo_diag_finish_f64")] == [3, 11, 8, 9, 10]

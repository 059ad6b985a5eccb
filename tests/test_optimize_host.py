"""CPU: the per-chain arithmetic of the batched L-BFGS -- exoplanet_amd/csrc/exo_optimize_core.hpp compiled for the host
(tests/optimize_harness.cpp), in double -- against tests/golden/lbfgs_phase.npz: single calls of the two phases with the
state afterwards from the long double build (tests/make_optimize_golden.py).  Integers and statuses are exact; floats within
max(4 E_host, 16 ulp), E_host being the double build's own largest error when the fixture was written.  The kernels on the
same cases: tests/test_gpu_optimize.py."""
import os
import subprocess

import numpy as np
import pytest

import optimize_cases as K

ULP = 2.220446049250313e-16


@pytest.fixture(scope="module")
def lib():
    return K.harness()


@pytest.fixture(scope="module")
def gold():
    return K.load()


def test_fixture_covers_the_sizes_and_every_branch(gold, lib):
    cases, e_host = gold
    assert lib.harness_max_history() == 32
    assert sorted(cases) == sorted(K.cases()) and 0.0 < e_host < 64 * ULP
    assert {c["n"] for c, _ in cases.values()} == {1, 5, 13} and all(c["hs"].shape == (K.HIST, c["n"]) for c, _ in cases.values())
    assert os.path.getsize(K.GOLD) < 400_000
    stored = {c["m"] for c, w in cases.values() if c["phase"] == 1 and w["n_iter"] > c["n_iter"]}
    assert {0, 2, 3} <= stored
    # wrapped: a full history whose next slot is not the first
    assert any(c["m"] == K.HIST and c["head"] > 0 and w["head"] != c["head"] for c, w in cases.values())
    phase1 = [(c, w) for c, w in cases.values() if c["phase"] == 1 and c["status"] == 0]
    accept = [(c, w) for c, w in phase1 if w["n_iter"] == c["n_iter"] + 1]
    reject = [(c, w) for c, w in phase1 if w["n_iter"] == c["n_iter"]]
    assert any(w["head"] == c["head"] for c, w in accept)                                            # curvature skip
    assert any(w["m"] == 0 and c["m"] > 0 for c, w in accept)                                        # not a descent direction
    assert {w["status"] for _, w in accept} == {0, 1, 2}                                             # both stops
    assert any(w["n_rej"] == c["n_rej"] + 1 and w["status"] == 0 for c, w in reject)                 # plain reject
    assert any(c["m"] > 0 and w["m"] == 0 and w["n_rej"] == 0 for c, w in reject)                    # at the limit, with history
    assert any(w["status"] == 3 for c, w in reject)                                                  # at the limit, without
    assert any(not np.isfinite(c["lpt"]) for c, _ in reject) and any(not np.isfinite(c["gt"]).all() for c, _ in reject)
    assert {w["status"] for c, w in cases.values() if c["phase"] == 0} == {0, 1, 4}
    assert any(c["phase"] == 1 and c["status"] != 0 for c, _ in cases.values())                      # a chain that has stopped
    assert any((c["free"] == 0).any() for c, _ in cases.values())


def test_the_generator_still_makes_these_inputs(gold):
    cases, _ = gold
    for name, c in K.cases().items():
        for k, v in c.items():
            assert np.array_equal(np.asarray(v), np.asarray(cases[name][0][k]), equal_nan=True), (name, k)


@pytest.mark.parametrize("name", sorted(K.cases()))
def test_double_build_matches_the_fixture(name, lib, gold):
    cases, e_host = gold
    c, want = cases[name]
    got = K.run_harness(lib, c, long_double=False)
    assert {k: got[k] for k in K.INTS} == {k: want[k] for k in K.INTS}
    err = K.float_error(got, want)
    print(f"{name}: error {err:.2e} (E_host {e_host:.2e})")
    assert err <= max(4 * e_host, 16 * ULP)
    if c["phase"] == 1 and c["status"] != 0:          # a chain that has stopped: nothing of its state changes
        for k in K.FLOATS + K.INTS:
            if k != "gt":
                assert np.array_equal(np.asarray(got[k]), np.asarray(c[k])), k
    held = c["free"] == 0
    assert np.array_equal(got["xt"][held], c["x"][held]) and np.array_equal(got["x"][held], c["x"][held])


def test_no_decision_of_a_case_is_close(gold):
    cases, _ = gold
    for name, (c, want) in cases.items():
        m = K.margins(c, want)
        assert all(v > K.MARGIN for v in m.values()), (name, m)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """the harness with its own main (both phases until a chain stops, every array at its exact size), built with the address
    and undefined-behaviour sanitizers and run as a program"""
    exe = str(tmp_path / "optimize_harness_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DOPTIMIZE_HARNESS_MAIN", "-o", exe, os.path.join(K.ROOT, "tests", "optimize_harness.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.count("status") == 2

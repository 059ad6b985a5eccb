"""CPU: the arithmetic of the chain diagnostics -- exoplanet_amd/csrc/exo_diagnostics_core.hpp compiled for the host
(tests/diagnostics_harness.cpp), in double and in long double -- against tests/golden/diagnostics_mp.npz (mpmath at 40 digits,
tests/make_diagnostics_golden.py).  max_t and the NaN pattern are exact; floats within max(4 E_host, 16 ulp), E_host being
the double build's own largest error when the fixture was written.  The kernels on the same cases:
tests/test_gpu_diagnostics.py."""
import os
import subprocess

import numpy as np
import pytest

import diagnostics_cases as K


@pytest.fixture(scope="module")
def lib():
    return K.harness()


@pytest.fixture(scope="module")
def gold():
    return K.load()


def test_fixture_covers_the_shapes_and_kinds(gold, lib):
    cases, e_host = gold
    assert lib.harness_lag_block() == 16 and lib.harness_n_out() == len(K.COLUMNS)
    assert sorted(cases) == sorted(K.SHAPES) and 0.0 < e_host < 1e-9
    assert os.path.getsize(K.GOLD) < 1_000_000
    shapes = {(x.shape[1], x.shape[0]) for x, _ in cases.values()}
    assert {(1, 8), (3, 37), (4, 101), (33, 64), (130, 64), (64, 200), (2, 3)} == shapes
    assert set(K.ALL) == {k for _, _, _, kinds in K.SHAPES.values() for k in kinds}
    x, want = cases["c64_n200"]
    ar9 = K.SHAPES["c64_n200"][3].index("ar9")
    assert want["max_t_bulk"][ar9] > 3 * 16                       # truncation runs over several lag blocks
    arm5 = K.SHAPES["c64_n200"][3].index("arm5")
    assert want["ess_bulk"][arm5] > 64 * 200                      # antithetic: more than S
    for name, (C, N, _, kinds) in K.SHAPES.items():
        want = cases[name][1]
        for p, kind in enumerate(kinds):
            row = {k: want[k][p] for k in K.FLOATS}
            if kind == "nan" or N < 4:
                assert all(np.isnan(v) for v in row.values()) and all(want[k][p] == -1 for k in K.INTS), (name, kind)
            elif kind == "const":
                S = 2 * C * (N // 2)
                assert row["ess_bulk"] == row["ess_tail"] == row["ess_mean"] == S and np.isnan(row["r_hat"]) and row["sd"] == 0
            else:
                assert all(np.isfinite(v) for v in row.values()), (name, kind, row)
            if kind == "shifted" and C <= 4:                      # (one chain of a few: of 33 it moves R-hat by less)
                assert row["r_hat"] > 1.2


def test_the_generator_still_makes_these_inputs(gold):
    cases, _ = gold
    for name, x in K.cases().items():
        assert np.array_equal(x, cases[name][0], equal_nan=True), name


@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_double_build_matches_the_fixture(name, lib, gold):
    cases, e_host = gold
    x, want = cases[name]
    for long_double in (False, True):
        err = K.errors(K.run_harness(lib, x, long_double), want)
        print(f"{name} {'long double' if long_double else 'double'}: errors {err} (E_host {e_host:.2e})")
        assert max(err.values()) <= max(4 * e_host, 16 * K.ULP)


def test_normal_scores_of_the_extreme_ranks(lib):
    """Phi^-1 at the ends of a million ranks and in the middle, double against long double: the upper tail is formed from
    1 - p, so both ends are equally accurate"""
    S = 1 << 20
    for rank2 in (2, 3, 200, S // 2, S, S + 1, S + 2, 2 * S - 1, 2 * S):
        a, b = lib.harness_ndtri(0, rank2, S), lib.harness_ndtri(1, rank2, S)
        assert abs(a - b) <= 4 * K.ULP * max(abs(b), 1e-3), (rank2, a, b)
        assert lib.harness_ndtri(0, rank2, S) == -lib.harness_ndtri(0, 2 * (S + 1) - rank2, S)
    assert lib.harness_ndtri(0, S + 1, S) == 0.0
    # mpmath at 30 digits: Phi^-1(5 / 66), and the first of a million ranks
    assert abs(lib.harness_ndtri(0, 2, 8) - (-1.43420015968637945613)) < 4 * K.ULP * 1.5
    assert abs(lib.harness_ndtri(0, 2, S) - (-4.85694737267144854582)) < 4 * K.ULP * 4.9


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """the harness with its own main (an odd length, a single chain, several lag blocks; every array at its exact size), built
    with the address and undefined-behaviour sanitizers and run as a program"""
    exe = str(tmp_path / "diagnostics_harness_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DDIAGNOSTICS_HARNESS_MAIN", "-o", exe, os.path.join(K.ROOT, "tests", "diagnostics_harness.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.count("ess_bulk") == 6

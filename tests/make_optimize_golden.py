"""Writes tests/golden/lbfgs_phase.npz: the single-call cases of tests/optimize_cases.py -- the state of one chain before a
call of a phase of the batched L-BFGS -- with the state afterwards as the long double build of
exoplanet_amd/csrc/exo_optimize_core.hpp (tests/optimize_harness.cpp) computes it, rounded to double, and E_host: the largest
error of the double build against that (optimize_cases.float_error).  Asserts that every case takes the branch it is named
for and that no decision of a case hinges on less than optimize_cases.MARGIN, relative.

    python tests/make_optimize_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optimize_cases as K  # noqa: E402

# what the call of every case must leave: (status, n_iter, n_eval, m, head, n_rej, n_small)
EXPECT = {
    "start_n5": (0, 0, 1, 0, 0, 0, 0),
    "start_small_gradient_n1": (0, 0, 1, 0, 0, 0, 0),
    "start_big_gradient_n13": (0, 0, 1, 0, 0, 0, 0),
    "start_converged_n1": (1, 0, 1, 0, 0, 0, 0),
    "start_value_not_finite_n5": (4, 0, 1, 0, 0, 0, 0),
    "start_gradient_not_finite_n5": (4, 0, 1, 0, 0, 0, 0),
    "accept_first_pair_n5": (0, 5, 10, 1, 1, 0, 0),
    "accept_one_pair_n1": (0, 5, 10, 2, 2, 0, 0),
    "accept_two_pairs_n13": (0, 5, 10, 3, 0, 0, 0),
    "accept_full_history_n5": (0, 5, 10, 3, 1, 0, 0),
    "accept_wrapped_n13": (0, 5, 10, 3, 2, 0, 0),
    "accept_curvature_skip_n5": (0, 5, 10, 0, 2, 0, 0),
    "accept_curvature_skip_no_history_n13": (0, 5, 10, 0, 0, 0, 0),
    "accept_not_descent_n5": (0, 5, 10, 0, 1, 0, 0),
    "reject_n13": (0, 4, 10, 2, 1, 4, 0),
    "reject_limit_with_history_n5": (0, 4, 10, 0, 2, 0, 0),
    "reject_limit_without_history_n1": (3, 4, 10, 0, 0, 5, 0),
    "reject_limit_without_history_n5": (3, 4, 10, 0, 0, 20, 0),
    "stop_gradient_n5": (1, 5, 10, 3, 0, 0, 0),
    "stop_value_n13": (2, 5, 10, 3, 0, 0, 3),
    "stop_value_waits_n13": (0, 5, 10, 2, 2, 0, 2),
    "stop_value_waits_masked_n5": (0, 5, 10, 2, 2, 0, 2),
    "reject_limit_after_small_decrease_n5": (2, 4, 10, 0, 0, 20, 1),
    "trial_value_nan_n5": (0, 4, 10, 2, 2, 1, 0),
    "trial_gradient_inf_n13": (0, 4, 10, 3, 1, 1, 0),
    "stopped_chain_n5": (2, 4, 9, 2, 2, 0, 0),
}


def main():
    lib = K.harness()
    cases = K.cases()
    assert set(cases) == set(EXPECT), set(cases) ^ set(EXPECT)
    assert {c["n"] for c in cases.values()} == {1, 5, 13}
    arrays, e_host = {}, 0.0
    for name, c in cases.items():
        want = K.run_harness(lib, c, long_double=True)
        got = K.run_harness(lib, c, long_double=False)
        ints = tuple(want[k] for k in K.INTS)
        assert ints == EXPECT[name], (name, ints)
        assert all(got[k] == want[k] for k in K.INTS), name
        m = K.margins(c, want)
        assert all(v > K.MARGIN for v in m.values()), (name, m)
        err = K.float_error(got, want)
        e_host = max(e_host, err)
        print("%-40s error of the double build %.2e   margins %s" % (name, err, {k: "%.1e" % v for k, v in m.items()}))
        for k, v in c.items():
            arrays[f"{name}/in/{k}"] = np.asarray(v)
        for k in K.FLOATS + K.INTS:
            arrays[f"{name}/out/{k}"] = np.asarray(want[k])
    arrays["E_host"] = np.asarray(e_host)
    np.savez_compressed(K.GOLD, **arrays)
    print("E_host = %.3e; %d cases, %d bytes" % (e_host, len(cases), os.path.getsize(K.GOLD)))


if __name__ == "__main__":
    main()

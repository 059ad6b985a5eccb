"""CPU: the torch statement of exoplanet_amd.diagnostics -- what runs for CPU tensors, and the definition -- against
tests/golden/diagnostics_mp.npz under the rule the kernels are held to (tests/test_gpu_diagnostics.py): max_t and the NaN
pattern exact, floats within max(4 E_host, 16 ulp).  Sanity brackets on seeded inputs, the BFMI and the summary object."""
import numpy as np
import pytest
import torch

import diagnostics_cases as K
from exoplanet_amd import diagnostics as dg


@pytest.fixture(scope="module")
def gold():
    return K.load()


def _as_numpy(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_torch_statement_matches_the_fixture(name, gold):
    cases, e_host = gold
    x, want = cases[name]
    err = K.errors(_as_numpy(dg._torch_statement(torch.as_tensor(x))), want)
    print(f"{name}: errors {err} (E_host {e_host:.2e})")
    assert max(err.values()) <= max(4 * e_host, 16 * K.ULP)


def test_public_functions_return_one_value_per_event_element(gold):
    cases, _ = gold
    x, want = cases["c3_n37"]
    t = torch.as_tensor(x).reshape(37, 3, 2, 5)                     # an event of shape (2, 5)
    for got, key in ((dg.rhat(t), "r_hat"), (dg.ess(t), "ess_bulk"), (dg.ess(t, "tail"), "ess_tail"),
                     (dg.ess(t, "mean"), "ess_mean"), (dg.mcse_mean(t), "mcse_mean")):
        assert got.shape == (2, 5)
        np.testing.assert_allclose(got.reshape(-1).numpy(), want[key], rtol=1e-9, equal_nan=True)
    assert dg.rhat(t[:, :, 0, 0]).shape == ()
    with pytest.raises(ValueError):
        dg.ess(t, "median")
    with pytest.raises(TypeError):
        dg.rhat(t.float())


def _ar1(rng, N, C, phi):
    e = rng.standard_normal((N + 200, C))
    y = np.zeros_like(e)
    for n in range(1, N + 200):
        y[n] = phi * y[n - 1] + e[n]
    return y[200:]


def test_sanity_brackets_on_seeded_inputs():
    rng = np.random.default_rng(5)
    S = 64 * 200
    iid = torch.as_tensor(rng.standard_normal((200, 64)))
    assert 0.9 <= float(dg.ess(iid)) / S <= 1.1 and 0.99 <= float(dg.rhat(iid)) <= 1.01
    phi = 0.9
    ar = torch.as_tensor(_ar1(rng, 200, 64, phi))
    ratio = float(dg.ess(ar)) / S / ((1 - phi) / (1 + phi))
    print("AR(1) 0.9: ess_bulk / S = %.3f x (1 - phi) / (1 + phi)" % ratio)
    assert 0.5 <= ratio <= 1.5
    y = _ar1(rng, 100, 4, phi)
    y[:, 0] += 3 * y.std()
    assert float(dg.rhat(torch.as_tensor(y))) > 1.2


def test_degenerate_series_leave_their_neighbours_alone():
    rng = np.random.default_rng(6)
    x = torch.as_tensor(rng.standard_normal((50, 3, 4)))
    clean = dg._torch_statement(x)
    y = x.clone()
    y[7, 1, 1] = float("inf")
    y[:, :, 2] = -1.5
    got = dg._torch_statement(y)
    for k in K.FLOATS:
        assert torch.equal(got[k][[0, 3]], clean[k][[0, 3]]), k
        assert bool(torch.isnan(got[k][1]))
    assert float(got["ess_bulk"][2]) == float(got["ess_tail"][2]) == 150.0 and bool(torch.isnan(got["r_hat"][2]))
    assert all(bool(torch.isnan(v).all()) for k, v in dg._torch_statement(x[:3]).items() if k in K.FLOATS)
    one = dg._torch_statement(x[:, :1])                                 # a single chain: two half-chains
    assert bool(torch.isfinite(one["r_hat"]).all()) and bool((one["ess_bulk"] > 0).all())


def test_bfmi_and_summary():
    rng = np.random.default_rng(7)
    e = rng.standard_normal((300, 5))
    got = dg.bfmi(torch.as_tensor(e))
    want = (np.diff(e, axis=0) ** 2).mean(0) / e.var(0)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-13)
    assert got.shape == (5,) and bool(((got > 1.5) & (got < 2.5)).all())        # independent energies: 2
    theta = {"period": torch.as_tensor(rng.standard_normal((300, 5, 1))), "u": torch.as_tensor(rng.standard_normal((300, 5, 2)))}
    stats = dict(diverging=torch.zeros(300, 5, dtype=torch.bool), energy=torch.as_tensor(e),
                 accept_prob=torch.full((300, 5), 0.75, dtype=torch.float64), depth=torch.full((300, 5), 3.0, dtype=torch.float64))
    stats["diverging"][4, 2] = True
    s = dg.summary(theta, stats)
    assert s.names == ["period", "u[0]", "u[1]"] and s.n_divergent == 1 and s.mean_accept_prob == 0.75 and s.mean_depth == 3.0
    assert torch.equal(s.bfmi, got)
    d = s.to_dict()
    assert set(d["u[1]"]) == set(dg.Summary.columns) and d["_stats"]["n_divergent"] == 1
    assert abs(d["u[0]"]["sd"] - float(theta["u"][:, :, 0].std())) < 1e-12
    np.testing.assert_allclose(d["period"]["q95"], np.quantile(theta["period"].numpy(), 0.95), rtol=1e-13)
    text = str(s)
    assert "r_hat" in text and "ess_bulk" in text and "u[1]" in text and "divergent transitions: 1" in text
    plain = dg.summary(theta["u"])
    assert plain.names == ["x[0]", "x[1]"] and plain.n_divergent is None and "divergent" not in str(plain)

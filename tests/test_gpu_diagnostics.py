"""GPU: exoplanet_amd.diagnostics on the device -- the kernels of exo_diag_*_f64 against tests/golden/diagnostics_mp.npz
(mpmath at 40 digits), through the C ABI (`ops.chain_diagnostics`) and through the public functions: max_t and the NaN pattern
exact, floats within max(4 E_host, 16 ulp) -- the device and host builds of one header differ in their library functions
only.  Determinism, and the device path against the torch statement on the same tensor.

Measured on the MI355X (largest error per column over all cases, bound 1.66e-14): see DESIGN.md section 16.4."""
import numpy as np
import pytest
import torch

import diagnostics_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return K.load()


def _split(x, dev):
    """x (N, C, P) numpy -> (x_split (P, L, M), x_full or None, M) as `diagnostics._device` forms them"""
    t = torch.as_tensor(x, device=dev)
    N, C, P = t.shape
    L = N // 2
    xs = torch.cat([t[:L], t[N - L:]], dim=1).permute(2, 0, 1).contiguous()
    full = None if N % 2 == 0 else t.permute(2, 0, 1).reshape(P, N * C).contiguous()
    return xs, full, 2 * C


def test_kernels_against_the_fixture_through_the_c_abi(dev, gold):
    from exoplanet_amd import ops

    cases, e_host = gold
    tol = max(4 * e_host, 16 * K.ULP)
    worst, n_run = {}, 0
    for name, (x, want) in sorted(cases.items()):
        xs, full, M = _split(x, dev)
        if x.shape[0] < 4:
            # fewer than four draws: the library refuses the sizes, before any launch; what the caller answers instead is NaN
            # (the next test)
            with pytest.raises(ValueError):
                ops.chain_diagnostics(xs, full, M)
            assert all(np.isnan(want[k]).all() for k in K.FLOATS)
            n_run += 1
            continue
        info = {}
        out = ops.chain_diagnostics(xs, full, M, timings=info)
        err = K.errors(K.table(out.cpu().numpy()), want)
        assert info["lag_blocks"] <= -(-xs.shape[1] // 16)
        for k, v in err.items():
            worst[k] = max(worst.get(k, 0.0), v)
        n_run += 1
        print(f"{name}: {info['lag_blocks']} lag blocks, errors", {k: "%.1e" % v for k, v in err.items()})
    print("kernels, largest error per column:", {k: "%.2e" % v for k, v in worst.items()}, f"(E_host {e_host:.2e}, bound {tol:.2e})")
    assert n_run == len(cases) and max(worst.values()) <= tol


def test_public_functions_against_the_fixture(dev, gold):
    from exoplanet_amd import diagnostics as dg

    cases, e_host = gold
    tol = max(4 * e_host, 16 * K.ULP)
    worst = 0.0
    for name, (x, want) in sorted(cases.items()):                    # every case: N = 3 is answered with NaN
        t = torch.as_tensor(x, device=dev)
        res, event = dg._compute(t)
        assert event == (x.shape[2],) and all(v.is_cuda for v in res.values())
        got = {k: v.cpu().numpy() for k, v in res.items()}
        worst = max(worst, max(K.errors(got, want).values()))
        for fn, key in ((dg.rhat, "r_hat"), (dg.mcse_mean, "mcse_mean"), (lambda v: dg.ess(v, "tail"), "ess_tail")):
            assert np.array_equal(fn(t).cpu().numpy(), got[key], equal_nan=True)
    print(f"public functions: largest error {worst:.2e} (bound {tol:.2e})")
    assert worst <= tol


def test_same_input_same_bits_and_parameters_permute(dev, gold):
    from exoplanet_amd import ops

    cases, _ = gold
    for name in ("c33_n64", "c3_n37", "c64_n200"):
        x = cases[name][0]
        xs, full, M = _split(x, dev)
        a, b = ops.chain_diagnostics(xs, full, M), ops.chain_diagnostics(xs, full, M)
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)), name
        perm = torch.randperm(x.shape[2], generator=torch.Generator().manual_seed(3)).to(dev)
        c = ops.chain_diagnostics(xs[perm].contiguous(), None if full is None else full[perm].contiguous(), M)
        assert torch.equal(torch.nan_to_num(c, nan=-7.0), torch.nan_to_num(a[perm], nan=-7.0)), name


def test_device_path_against_the_torch_statement(dev, gold, monkeypatch):
    from exoplanet_amd import diagnostics as dg

    cases, e_host = gold
    tol = max(4 * e_host, 16 * K.ULP)
    worst = 0.0
    for name, (x, _) in sorted(cases.items()):
        t = torch.as_tensor(x, device=dev)
        got = {k: v.cpu().numpy() for k, v in dg._compute(t)[0].items()}
        ref = {k: v.numpy() for k, v in dg._compute(t.cpu())[0].items()}
        worst = max(worst, max(K.errors(got, ref).values()))
    print(f"device path against the torch statement on the CPU: largest difference {worst:.2e} (bound {tol:.2e})")
    assert worst <= tol
    # parameters in several library calls: the same bits as in one
    t = torch.as_tensor(cases["c33_n64"][0], device=dev)
    one = dg._compute(t)[0]
    monkeypatch.setattr(dg, "_SET_BYTES", 3 * 8 * 5 * t.shape[0] * t.shape[1])      # three parameters per call
    for k, v in dg._compute(t)[0].items():
        assert torch.equal(torch.nan_to_num(v.double(), nan=-7.0), torch.nan_to_num(one[k].double(), nan=-7.0)), k
    s = dg.summary(t)
    assert len(s.names) == t.shape[2] and "ess_bulk" in str(s)

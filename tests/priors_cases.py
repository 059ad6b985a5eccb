"""The spaces of tests/golden/priors.npz, shared by the script that writes the fixture (tools/make_priors_golden.py, mpmath)
and the tests that read it.  A case is a list of (block name, constructor name, positional arguments, keyword arguments)."""
import numpy as np

CASES = {
    "normal": [("a", "normal", (3.5, 0.01), {}), ("l", "lognormal", (0.1, 0.5), {"shape": (2,)})],
    "uniform_impact": [("r", "uniform", (0.01, 0.3), {"shape": (2,)}), ("b", "impact_parameter", ("r",), {"shape": (2,)}),
                       ("r1", "lognormal", (-2.0, 0.3), {}), ("b1", "impact_parameter", ("r1",), {"shape": (2,)}),
                       ("bc", "impact_parameter", (0.1,), {})],
    "angle": [("w", "angle", (), {}), ("v", "angle", (), {"regularization": None})],
    "unit_disk": [("h", "unit_disk", (), {})],
    "quad_limb_dark": [("u", "quad_limb_dark", (), {})],
    "kipping13": [("e", "kipping13", (), {}), ("es", "kipping13", (), {"long": False}), ("el", "kipping13", (), {"long": True})],
    "kipping13_bounded": [("e", "kipping13", (), {"lower": 0.1, "upper": 0.8}), ("es", "kipping13", (), {"long": False, "upper": 0.5}),
                          ("el", "kipping13", (), {"lower": 0.2})],
    "vaneylen19": [("e", "vaneylen19", (), {}), ("em", "vaneylen19", (), {"multi": True})],
    "vaneylen19_bounded": [("e", "vaneylen19", (), {"upper": 0.5}), ("em", "vaneylen19", (), {"multi": True, "lower": 0.1, "upper": 0.9})],
    "kipping13_free": [("e", "kipping13", (), {"fixed": False, "shape": (2,)}), ("es", "kipping13", (), {"fixed": False, "long": False})],
    "vaneylen19_free": [("e", "vaneylen19", (), {"fixed": False, "shape": (2,)}),
                        ("em", "vaneylen19", (), {"fixed": False, "multi": True, "lower": 0.05, "upper": 0.6})],
}

N_ROWS = 72
HYPER_COUNT = {"kipping13": 2, "vaneylen19": 3}
HYPER_CENTRE = {"kipping13": lambda kw: [np.log(0.697 if kw.get("long") is False else 1.12), np.log(3.27 if kw.get("long") is False else 3.09)],
                "vaneylen19": lambda kw: [np.log(0.049), np.log(0.26), np.log(0.08 / 0.92) if kw.get("multi") else np.log(0.76 / 0.24)]}


def build(xd, case):
    return xd.ParameterSpace(**{name: getattr(xd, ctor)(*args, **kw) for name, ctor, args, kw in CASES[case]})


def z_grid(case, seed):
    """N_ROWS points per case: normal draws of width 3, then rows that put every element coordinate at +-36, +-20, +-8 in turn
    and all at once.  A normal or lognormal block's coordinate stays within a few widths of its mean and a hyperparameter's within a factor e^1.5 of its
    prior's centre (exp(36) as the shape parameter of a Beta distribution is finite but says nothing about accuracy)."""
    rs = np.random.RandomState(seed)
    centre, width, free = [], [], []
    for name, ctor, args, kw in CASES[case]:
        count = (kw.get("shape") or (1,))[0]
        if not kw.get("fixed", True):
            c = HYPER_CENTRE[ctor](kw)
            centre += c; width += [0.5] * len(c); free += [False] * len(c)
        n = count * (2 if ctor in ("angle", "unit_disk", "quad_limb_dark") else 1)
        if ctor in ("normal", "lognormal"):
            centre += [args[0]] * n; width += [3 * args[1]] * n; free += [False] * n
        else:
            centre += [0.0] * n; width += [3.0] * n; free += [True] * n
    centre, width, free = np.array(centre), np.array(width), np.array(free)
    z = centre + width * rs.randn(N_ROWS, centre.size)
    row = N_ROWS - 1
    for big in (36.0, 20.0, 8.0):
        for sign in (1.0, -1.0):
            z[row, free] = sign * big
            row -= 1
            for k in np.flatnonzero(free)[:4]:
                z[row, k] = sign * big
                row -= 1
    return z

#!/usr/bin/env python
"""Writes tests/golden/contact_mp.npz: first / fourth contact and the in-transit windows of the geometries of
tests/contact_cases.py, with mpmath at 50 digits from the DEFINITION in the true anomaly f (tests/contact_cases.py, module
docstring) -- an outward scan from the conjunction for the first sign change of Delta^2 - L^2, mp.findroot on that bracket,
E on the branch continuous with f -- not from the kernels' theta or sin theta forms.  Nothing of the package or of
oracle/numpy_port.py is imported.  The scan is run at SCAN and at 2 SCAN steps per quarter turn; the two must agree in every
stored number (asserted, and said in the output).

    python tools/make_contact_golden.py          (under a minute on 8 cores; --check: compare with the committed file, write nothing)

Arrays (E entries, float64 unless noted; NaN where an entry has no such number):
  names (E,) str   ctor (E, 10) EXO_IN_* constructor inputs   inputs (E, 7) a, e, cos w, sin w, cos i, sin i, L
  circular, sec (E,) int8
  -- contact level: functions of ``inputs`` --
  flag (E,) int32   margin (E,) |Delta^2(f_c) - L^2| / L^2   M, theta, gprime, T, dMdf, Eterm (E, 2): left, right
  -- window level: functions of ``ctor`` (the constructor's algebra in mpmath; circular entries as e = 0, omega = 0) --
  w_flag (E, 2) int32 transit, occultation   fallback (E,) int8: lo >= 0 and hi <= P fails
  win (E, 4) ts, te, ts2, te2 (-inf / +inf where there is no contact or the fallback applies)
  w_gprime, w_T, w_Tin, w_dMdf, w_Eterm, w_E0term, w_theta (E, 4)
  circ_x, circ_arg, circ_hdur (E,)   circ_win (E, 4): Winn (2010) eq. 14, NaN where arg < 0 or x > 1
  -- cadences of every entry with contacts, placed from win (circular entries: circ_win) --
  cad_t (E, 64) sorted   cad_in (E, 64) int8: 0 outside, 1 in transit, 2 in occultation
  cad_margin (E, 64): distance in days to the nearest contact, of the float64 cadence
  cad_depth (E, 64): L - Delta(t) in R_star of the cadences inside a window (Kepler's equation in mpmath): how far the disks overlap
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_cases as K  # noqa: E402

mp.mp.dps = 50
SCAN = 512
F = mp.mpf
NAN = float("nan")


def solve(a, e, w, ci, si, L, scan, cw=None, sw=None):
    """dict(flag, margin, and per side M, theta, gprime, T, Tin, dMdf, Eterm) of the contacts about f_c = pi/2 - w"""
    p = a * (1 - e) * (1 + e)
    cw = mp.cos(w) if cw is None else cw
    sw = mp.sin(w) if sw is None else sw
    fc = mp.pi / 2 - w

    def parts(th):
        f = fc + th
        D = 1 + e * mp.cos(f)
        rho = p / D
        q = 1 - si * si * mp.sin(w + f) ** 2
        return f, D, rho, q

    def g(th):
        f, D, rho, q = parts(th)
        return rho * rho * q - L * L

    g0 = g(F(0))
    out = dict(flag=0 if g0 < 0 else 1, margin=float(abs(g0) / (L * L)), M=[NAN, NAN], theta=[NAN, NAN], gprime=[NAN, NAN],
               T=[NAN, NAN], Tin=[NAN, NAN], dMdf=[NAN, NAN], Eterm=[NAN, NAN], closest=float(abs(g0) / (L * L)))
    if out["flag"]:
        return out
    sides = []
    for sgn in (-1, 1):
        lo, hi = F(0), None
        closest = abs(g0)
        for k in range(1, scan + 1):
            th = sgn * k * (mp.pi / 2) / scan
            gk = g(th)
            if gk > 0:
                hi = th
                break
            closest = min(closest, -gk)
            lo = th
        if hi is None:
            out["flag"] = 1
            out["closest"] = float(closest / (L * L))
            return out
        root = mp.findroot(g, (lo, hi), solver="illinois", tol=mp.mpf(10) ** -90, maxsteps=400)
        assert min(lo, hi) <= root <= max(lo, hi) and abs(g(root)) < mp.mpf(10) ** -40 * L * L
        f, D, rho, q = parts(root)
        half = f / 2
        E = 2 * mp.atan2(mp.sqrt(1 - e) * mp.sin(half), mp.sqrt(1 + e) * mp.cos(half))
        E += 2 * mp.pi * mp.nint((f - E) / (2 * mp.pi))
        assert abs(f - E) < mp.pi
        M = E - e * mp.sin(E)
        T = rho * rho * q * (1 + 2 * e * (abs(sw * mp.cos(root)) + abs(cw * mp.sin(root))) / D) + L * L
        sides.append(dict(M=M, theta=root, gprime=abs(mp.diff(g, root)), T=T, Tin=rho * rho * q,
                          dMdf=((1 - e) * (1 + e)) ** F(1.5) / (D * D), Eterm=abs(E) + e * abs(mp.sin(E))))
    for key in ("M", "theta", "gprime", "T", "Tin", "dMdf", "Eterm"):
        out[key] = [sides[0][key], sides[1][key]]
    return out


def wrap_half(x, P):
    """x + P/2 mod P - P/2  (keplerian.py:755-759)"""
    hp = P / 2
    return (x + hp) - P * mp.floor((x + hp) / P) - hp


def entry(args):
    idx, scan = args
    c = K.CASES[idx]
    ct = K.ctor_inputs(c)
    inp = K.contact_inputs(ct)
    r = dict(ctor=ct, inputs=inp, circular=int(c["ecc"] is None), sec=int(c["sec"]))
    # ---- contact level: the seven float64 numbers
    # (sin^2 i = 1 - cos^2 i of the float64 cos i: no implementation reads the sin i it is handed -- 1 - sin^2 i sin^2(w + f) is
    # a cancelling difference at the size of rho^2 / L^2 roundings of sin i, up to 3e7 here, that belongs to nobody's solver)
    a, e, cw, sw, ci, si, L = [F(float(x)) for x in inp]
    si = mp.sqrt(max(F(0), 1 - ci * ci))
    s = solve(a, e, mp.atan2(sw, cw), ci, si, L, scan)
    r.update(flag=s["flag"], margin=s["margin"], closest=s["closest"])
    for key in ("M", "theta", "gprime", "T", "dMdf", "Eterm"):
        r[key] = [float(x) for x in s[key]]
    # ---- window level: the constructor's algebra in mpmath
    P, t0, b, e, w, rp, ms, rs, mpl, sbr = [F(float(x)) for x in ct]
    a = mp.cbrt(F(K.G_GRAV) * (ms + mpl) * P * P / (4 * mp.pi ** 2))
    n = 2 * mp.pi / P
    ci = (1 + e * mp.sin(w)) / ((1 - e) * (1 + e)) * rs / a * b
    si = mp.sqrt(max(F(0), 1 - ci * ci))
    L = rs + rp
    win = [-mp.inf, mp.inf, -mp.inf, mp.inf]
    w_flag, fallback = [1, 1], 0
    terms = {k: [NAN] * 4 for k in ("gprime", "T", "Tin", "dMdf", "Eterm", "E0term", "theta")}

    def M0_of(wk):
        E0 = 2 * mp.atan2(mp.sqrt(1 - e) * mp.cos(wk), mp.sqrt(1 + e) * (1 + mp.sin(wk)))
        return E0 - e * mp.sin(E0), abs(E0) + e * abs(mp.sin(E0))

    M0, E0term = M0_of(w)
    closest = r["closest"]
    if abs(ci) <= 1:
        s = solve(a, e, w, ci, si, L, scan)
        w_flag[0] = s["flag"]
        closest = min(closest, s["closest"])
        if not s["flag"]:
            a0, a1 = wrap_half((s["M"][0] - M0) / n, P), wrap_half((s["M"][1] - M0) / n, P)
            win[0] = a0 - P if a0 > 0 else a0
            win[1] = a1 + P if a1 < 0 else a1
            for k in ("gprime", "T", "Tin", "dMdf", "Eterm", "theta"):
                terms[k][0:2] = s[k]
            terms["E0term"][0:2] = [E0term, E0term]
        if True:   # (the occultation window of every entry: FLAG_SECONDARY is a flag of the whole call)
            M02, E02term = M0_of(w - mp.pi)
            s = solve(a, e, w - mp.pi, ci, si, L, scan)
            w_flag[1] = s["flag"]
            closest = min(closest, s["closest"])
            if not s["flag"]:
                a0, a1 = wrap_half((s["M"][0] - M02) / n, P), wrap_half((s["M"][1] - M02) / n, P)
                s0 = a0 - P if a0 > 0 else a0
                s1 = a1 + P if a1 < 0 else a1
                shift = (M02 - M0) / n
                shift = shift - P * mp.floor(shift / P)
                lo, hi = shift + s0, shift + s1
                if lo >= 0 and hi <= P:
                    win[2], win[3] = lo, hi
                    for k in ("gprime", "T", "Tin", "dMdf", "Eterm", "theta"):
                        terms[k][2:4] = s[k]
                    terms["E0term"][2:4] = [E02term + E0term + E02term] * 2
                else:
                    fallback = 1
    r.update(w_flag=w_flag, fallback=fallback, win=[float(x) for x in win], closest=closest)
    for k, v in terms.items():
        r["w_" + k] = [float(x) for x in v]
    # ---- the circular closed form, Winn (2010) eq. 14 / keplerian.py:733-741
    r.update(circ_x=NAN, circ_arg=NAN, circ_hdur=NAN, circ_win=[NAN] * 4)
    cwin = None
    if c["ecc"] is None:
        kk = rp / rs
        arg = (1 + kk) ** 2 - b * b
        cic = rs * b / a
        sic = mp.sqrt(max(F(0), 1 - cic * cic))
        r["circ_arg"] = float(arg)
        if arg >= 0 and sic > 0:
            x = rs / (a * sic) * mp.sqrt(arg)
            r["circ_x"] = float(x)
            if x <= 1:
                hdur = (P / 2) * mp.asin(x) / mp.pi
                r["circ_hdur"] = float(hdur)
                cwin = [-hdur, hdur, P / 2 - hdur, P / 2 + hdur]
                r["circ_win"] = [float(v) for v in cwin]
                # the closed form is the contact definition of a circular orbit
                assert not w_flag[0] and abs(win[1] - hdur) < mp.mpf(10) ** -35 * P and abs(win[0] + hdur) < mp.mpf(10) ** -35 * P
    # ---- cadences
    use = cwin if c["ecc"] is None else (win if not w_flag[0] else None)
    r.update(cad_t=[NAN] * K.N_CAD, cad_in=[0] * K.N_CAD, cad_margin=[NAN] * K.N_CAD, cad_depth=[NAN] * K.N_CAD)
    if use is not None:
        has2 = bool(c["sec"]) and mp.isfinite(use[2])      # ``sec``: the entry's cadences cover the occultation too
        epochs = (0, 1, 5) if has2 else (0, 1, 2, 5, 7, 11)
        ts = []
        for ep in epochs:
            base = t0 + ep * P
            for lo, hi in ((use[0], use[1]),) + (((use[2], use[3]),) if has2 else ()):
                dur = hi - lo
                for edge in (lo, hi):
                    for d in (F("1e-3"), F("1e-6")):
                        ts += [base + edge - d * dur, base + edge + d * dur]
                ts.append(base + (lo + hi) / 2)

        def where(t):
            dt = wrap_half(t - t0, P)
            ph = (t - t0) - P * mp.floor((t - t0) / P)
            inside = 1 if use[0] <= dt <= use[1] else (2 if has2 and use[2] <= ph <= use[3] else 0)
            m = min(abs(dt - use[0]), abs(dt - use[1]))
            if has2:
                m = min(m, abs(ph - use[2]), abs(ph - use[3]))
            return inside, m

        far = []
        dur = use[1] - use[0]
        for j in range(40):
            t = t0 + 3 * P + (F(j) + F("0.5")) / 40 * P
            inside, m = where(t)
            if not inside and m > dur / 1000:
                far.append(t)
        far = far[:: max(1, len(far) // 10)][:10]
        ts += far
        while len(ts) < K.N_CAD:
            ts.append(t0 + (len(ts) + 13) * P + (use[0] + use[1]) / 2)
        tf = np.sort(np.array([float(t) for t in ts[:K.N_CAD]]))
        info = [where(F(float(t))) for t in tf]

        def depth(t):
            """L - Delta at time t, in R_star: Kepler's equation on the bracket [M - e, M + e]"""
            ee, ww = (F(0), F(0)) if c["ecc"] is None else (e, w)
            cc = rs * b / a if c["ecc"] is None else ci
            M = (t - t0) * n + (mp.pi / 2 if c["ecc"] is None else M0)
            E = M if ee == 0 else mp.findroot(lambda x: x - ee * mp.sin(x) - M, (M - ee, M + ee), solver="illinois",
                                              tol=mp.mpf(10) ** -80, maxsteps=500)
            f = 2 * mp.atan2(mp.sqrt(1 + ee) * mp.sin(E / 2), mp.sqrt(1 - ee) * mp.cos(E / 2))
            rho = a * (1 - ee * mp.cos(E))
            return (L - rho * mp.sqrt(1 - (1 - cc * cc) * mp.sin(ww + f) ** 2)) / rs

        deps = [float(depth(F(float(t)))) if i else NAN for t, (i, _) in zip(tf, info)]
        assert all(d > 0 for d, (i, _) in zip(deps, info) if i), c["name"]
        r.update(cad_t=tf.tolist(), cad_in=[i for i, _ in info], cad_margin=[float(m) for _, m in info], cad_depth=deps)
    return r


def main():
    E = len(K.CASES)
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        coarse = pool.map(entry, [(i, SCAN) for i in range(E)], chunksize=4)
        fine = pool.map(entry, [(i, 2 * SCAN) for i in range(E)], chunksize=4)
    keys = [k for k in coarse[0] if k != "closest"]
    for i, (x, y) in enumerate(zip(coarse, fine)):
        for k in keys:
            assert np.array_equal(np.asarray(x[k], dtype=float), np.asarray(y[k], dtype=float), equal_nan=True), (K.NAMES[i], k)
    print(f"scan of {SCAN} steps per quarter turn and of {2 * SCAN}: all {E} entries identical in every stored number")
    out = dict(names=np.array(K.NAMES))
    ints = dict(circular=np.int8, sec=np.int8, flag=np.int32, w_flag=np.int32, fallback=np.int8, cad_in=np.int8)
    for k in keys:
        out[k] = np.array([x[k] for x in fine], dtype=ints.get(k, np.float64))
    flag, wf = out["flag"], out["w_flag"]
    none = (flag != 0)
    worst = min(min(x["margin"], x["closest"]) for x, f in zip(fine, none) if f)
    print(f"entries {E}: with contacts {int((~none).sum())}, without {int(none.sum())} (smallest mp margin {worst:.3g}); "
          f"window level: transit windows {int((wf[:, 0] == 0).sum())}, occultation windows {int(np.isfinite(out['win'][:, 2]).sum())}, "
          f"boundary fallbacks {int(out['fallback'].sum())}, circular {int(out['circular'].sum())} "
          f"(degenerate {int((out['circular'] == 1).sum() - np.isfinite(out['circ_hdur']).sum())})")
    assert (~none).sum() >= 150 and none.sum() >= 20 and worst > 1e-9
    # the flag of the window level agrees with the contact level wherever both are asked
    assert np.array_equal(wf[:, 0] != 0, none), [K.NAMES[i] for i in np.nonzero((wf[:, 0] != 0) != none)[0]]
    for i, c in enumerate(K.CASES):
        assert not c["flag"] or none[i] or (c["ecc"] is None and not np.isfinite(out["circ_hdur"][i])), c["name"]
    path = os.path.join(K.GOLD, "contact_mp.npz")
    if "--check" in sys.argv:
        have = np.load(path)
        assert sorted(have.files) == sorted(out) and all(have[k].dtype == out[k].dtype and have[k].tobytes() == out[k].tobytes()
                                                          for k in out), "the committed fixture differs"
        print("every array of", path, "reproduced bit for bit")
        return
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

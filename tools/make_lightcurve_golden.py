#!/usr/bin/env python
"""Writes tests/golden/lightcurve_mp.npz: the light-curve flux of the systems of tests/lightcurve_mp_cases.py as a function
of the kernel's float64 record and limb-darkening vector, with its derivative to every gradient slot of the record and to c,
computed with mpmath at 40 digits by oracle/mp_lightcurve.py (record_sample: the reference's formulas on the record's slots;
dF/d(b, r) from the boundary integrals of oracle/mp_reference.py, d(b, r)/d slot from mpmath.diff of the orbit algebra,
never through the quadrature).  Neither the package nor oracle/numpy_port.py takes part in any number written here (the table
module is imported for its table alone).

    python tools/make_lightcurve_golden.py          (about half a minute on 8 cores; regenerates the file bit for bit)

The record of an entry is built from the table's user inputs with the mpmath Orbit of oracle/mp_lightcurve.py and rounded to
float64 ONCE; everything stored is a function of those rounded numbers.  Arrays (float64 unless noted), S entries:
  rec (S, 20)   c (S, 6)   secondary, grad, group (S,)   texp (S,)  n_sub (S,) int  sdt, sw (S, 7)
  ttv_n (S,) int (0 or 3 bins)  ttv_edges (S, 2)  ttv_shift (S, 3): a time t acts as t - ttv_shift[searchsorted(edges, t)]
  t_in (S, 20)  flux (S, 20)  jac_rec (S, 20, 11)  jac_c (S, 20, 6)  b_in (S, 20)     t_out (S, 16)
  user_in (S, 10)  user_u (S, 4)  jac_user (S, 11, 10)  jac_cu (S, 6, 4): the packing inputs (period, t0, b, ecc, omega, r, m_star,
  r_star, m_planet, sbr) and (u1, u2, u1s, u2s), d record / d input (rows in jac_rec's column order) and d c / d u, by
  mpmath.diff of Orbit.__init__ and get_cl; zeros for an entry no user-level call reproduces (t_periastron given).
  pk_in (K, 10)  pk_u (K, 2)  pk_rec (K, 11)  pk_jac (K, 11, 10): the same for the packing-only entries at e = 1 - 1e-8, 1 - 1e-6.
jac_rec columns: n, t_periastron, e, cos w, sin w, cos i, a/R, r/R, flux ratio (oracle.numpy_port.GRAD_SLOTS), then sin i and
c / R_star (non-zero only for the light-delay entries, whose record carries the speed of light).
Asserted per entry: |cos i| < 1; min flux < -1e-4; at least two cadences on each limb (|b - 1| < r); every t_out sample has
b > 1 + r + 1e-3 or the body behind the star with no occultation asked for.
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import mp_lightcurve as L  # noqa: E402

DPS = 40
mp.mp.dps = DPS
NPAR = 20
(P_N, P_TP, P_ECC, P_COSW, P_SINW, P_COSI, P_SINI, P_AOR, P_ROR, P_T0, P_PERIOD, P_TS, P_TE, P_FRATIO, P_TS2, P_TE2,
 P_CLIGHT) = range(17)          # include/exoplanet_amd.h


def table():
    import importlib.util

    spec = importlib.util.spec_from_file_location("lc_cases_table", os.path.join(ROOT, "tests", "lightcurve_mp_cases.py"))
    # only the table is wanted: the module's tolerance helpers import the oracle lazily
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------------------
# record of an entry
# ------------------------------------------------------------------------------------------------------------------------
def build_record(s):
    f = mp.mpf
    kw = dict(period=s["period"], b=s["b"], m_star=s["m_star"], r_star=s["r_star"], m_planet=s["m_planet"])
    if s["ecc"] is not None:
        kw.update(ecc=s["ecc"], omega=f(s["omega"]))
    if s["tp"] is not None:
        o = L.Orbit(t_periastron=s["tp"], **kw)
        # the transit nearest ``at``
        k = mp.nint((f(s["at"]) - o.t0) / o.period)
        t0 = o.t0 + k * o.period
    else:
        o = L.Orbit(t0=s["t0"], **kw)
        t0 = o.t0
    assert abs(o.cos_incl) < 1, s["name"]
    rec = np.zeros(NPAR)
    rec[[P_N, P_TP, P_ECC, P_COSW, P_SINW, P_COSI, P_SINI, P_AOR, P_ROR, P_T0, P_PERIOD]] = [
        float(v) for v in (o.n, o.t_periastron, 0 if o.ecc is None else o.ecc, o.cw, o.sw, o.cos_incl, o.sin_incl,
                           o.a / o.r_star, f(s["r"]) / o.r_star, t0, o.period)]
    rec[[P_TS, P_TS2]] = -np.inf
    rec[[P_TE, P_TE2]] = np.inf
    c = np.zeros(6)
    c[:3] = [float(v) for v in L.get_cl(*s["u"])]
    if s["sbr"] is not None:
        rec[P_FRATIO] = float(f(s["sbr"]) * (f(s["r"]) / o.r_star) ** 2)
        c[3:] = [float(v) for v in L.get_cl(*s["u2"])]
    if s["light_delay"]:
        rec[P_CLIGHT] = float(L.C_LIGHT / o.r_star)
    return rec, c


def user_record(x, circular, secondary):
    """the record's slots in the fixture's column order (n, tp, e, cw, sw, ci, aor, ror, fr, si, c / R_star) as a function of
    the packing inputs x = (period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr): Orbit.__init__ of oracle/mp_lightcurve"""
    period, t0, b, ecc, omega, r, m_star, r_star, m_planet, sbr = x
    kw = {} if circular else dict(ecc=ecc, omega=omega)
    o = L.Orbit(period=period, t0=t0, b=b, m_star=m_star, r_star=r_star, m_planet=m_planet, **kw)
    ror = r / o.r_star
    return [o.n, o.t_periastron, mp.mpf(0) if circular else o.ecc, o.cw, o.sw, o.cos_incl, o.a / o.r_star, ror,
            (sbr * ror * ror) if secondary else mp.mpf(0), o.sin_incl, L.C_LIGHT / o.r_star]


def user_jacobian(arg):
    """(record [11], d record / d input [11, 10], d c / d (u1, u2) [3, 2]) by mpmath.diff, every input in turn"""
    mp.mp.dps = DPS
    x, circular, secondary, u = arg
    xm = [mp.mpf(float(v)) for v in x]
    rec = user_record(xm, circular, secondary)
    J = np.zeros((11, 10))
    for k in range(10):
        if circular and k in (3, 4):
            continue
        seen = {}

        def at(v, k=k, seen=seen):
            if v not in seen:
                seen[v] = user_record(xm[:k] + [v] + xm[k + 1:], circular, secondary)
            return seen[v]
        for j in range(11):
            J[j, k] = float(mp.diff(lambda v, j=j: at(v)[j], xm[k]))
    um = [mp.mpf(float(v)) for v in u]
    Jc = np.zeros((3, 2))
    for k in range(2):
        for j in range(3):
            Jc[j, k] = float(mp.diff(lambda v, j=j, k=k: L.get_cl(*(um[:k] + [v] + um[k + 1:]))[j], um[k]))
    return np.array([float(v) for v in rec]), J, Jc


def mp_record(rec):
    f = mp.mpf
    return dict(n=f(rec[P_N]), tp=f(rec[P_TP]), e=f(rec[P_ECC]), cw=f(rec[P_COSW]), sw=f(rec[P_SINW]), ci=f(rec[P_COSI]),
                si=f(rec[P_SINI]), aor=f(rec[P_AOR]), ror=f(rec[P_ROR]), fr=f(rec[P_FRATIO]), cl=f(rec[P_CLIGHT]))


# ------------------------------------------------------------------------------------------------------------------------
# cadences
# ------------------------------------------------------------------------------------------------------------------------
def b_and_side(t, q, sigma=1):
    """(b, in front) of the body as seen at t; a record with a speed of light is seen with its delay (sigma: mp_lightcurve)"""
    b, y1 = L._seen(mp.mpf(t), q, q["e"] == 0, sigma, q["cl"] != 0, None)
    return b, -q["si"] * y1 > 0


def conjunction(rec, q, occultation):
    """time of the conjunction nearest the record's t0 (or half an orbit later in phase): true anomaly pi/2 - w, 3 pi/2 - w"""
    w = mp.atan2(q["sw"], q["cw"])
    fa = (3 if occultation else 1) * mp.pi / 2 - w
    e = q["e"]
    E = 2 * mp.atan2(mp.sqrt(1 - e) * mp.sin(fa / 2), mp.sqrt(1 + e) * mp.cos(fa / 2))
    tc = q["tp"] + (E - e * mp.sin(E)) / q["n"]
    period = 2 * mp.pi / q["n"]
    ref = mp.mpf(rec[P_T0]) + (period / 2 if occultation else 0)
    return tc + mp.nint((ref - tc) / period) * period


def crossing(q, t_inside, t_outside, level, sigma=1):
    """bisection for b(t) = level between a time with b < level and one with b > level"""
    lo, hi = mp.mpf(t_inside), mp.mpf(t_outside)
    for _ in range(70):
        mid = (lo + hi) / 2
        if b_and_side(mid, q, sigma)[0] < level:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def contacts(rec, q, occultation):
    """(t1, t2, t3, t4, tc): b = 1 + ror at t1, t4; b = |1 - ror| at t2, t3 (None, None where the body never gets inside)"""
    tc = conjunction(rec, q, occultation)
    ror = q["ror"]
    e = q["e"]
    sgn = sigma = -1 if occultation else 1
    est = (1 + ror) / (q["n"] * q["aor"]) * mp.sqrt((1 - e) * (1 + e)) / (1 + sgn * e * q["sw"])    # half duration, roughly
    # the closest approach lies near tc: walk outwards from it
    fine = [tc + est * mp.mpf(k) / 40 for k in range(-40, 41)]
    tmin = min(fine, key=lambda x: b_and_side(x, q, sigma)[0])
    bmin = b_and_side(tmin, q, sigma)[0]
    assert bmin < 1 + ror

    def walk(level, direction):
        step = est / 25
        x = tmin
        for _ in range(400):
            x = x + direction * step
            if b_and_side(x, q, sigma)[0] > level:
                return crossing(q, x - direction * step, x, level, sigma)
        raise AssertionError("no contact found")

    inner = abs(1 - ror)
    t1, t4 = walk(1 + ror, -1), walk(1 + ror, 1)
    t2, t3 = (walk(inner, -1), walk(inner, 1)) if bmin < inner else (None, None)
    return t1, t2, t3, t4, tmin


def pick(con, n_limb, n_int, beyond):
    """cadences of one event: n_limb on either limb, n_int between (uneven fractions, never the exact centre), and
    ``beyond`` (0, 1 or 2) just outside the outer contacts"""
    t1, t2, t3, t4, _ = con
    half = (t4 - t1) / 2
    out = []
    if beyond >= 1:
        out.append(t1 - half * mp.mpf("0.021"))
    if beyond >= 2:
        out.append(t4 + half * mp.mpf("0.017"))
    if t2 is None:
        m = 2 * n_limb + n_int
        out += [t1 + (t4 - t1) * (mp.mpf(k) + mp.mpf("0.43")) / m for k in range(m)]
        return out
    out += [t1 + (t2 - t1) * (mp.mpf(k) + mp.mpf("0.37")) / n_limb for k in range(n_limb)]
    out += [t3 + (t4 - t3) * (mp.mpf(k) + mp.mpf("0.61")) / n_limb for k in range(n_limb)]
    out += [t2 + (t3 - t2) * (mp.mpf(k) + mp.mpf("0.29")) / n_int for k in range(n_int)]
    return out


def times_of(entries, recs, K):
    """(t_in [N_IN], t_out [N_OUT]) shared by the entries of one unit, as float64"""
    qs = [mp_record(r) for r in recs]
    s0 = entries[0]
    t_in, cons = [], []
    if len(entries) > 1:
        assert len(entries) == 3 and K.N_IN == 20
        for k, (rec, q) in enumerate(zip(recs, qs)):
            con = contacts(rec, q, False)
            cons.append(con)
            t_in += pick(con, 2, 2, 2 if k == 0 else 0)
    elif s0["sbr"] is not None:
        for occ in (False, True):
            con = contacts(recs[0], qs[0], occ)
            cons.append(con)
            t_in += pick(con, 2, 5, 1)
    else:
        con = contacts(recs[0], qs[0], False)
        cons.append(con)
        t_in += pick(con, 3, 12, 2)
    assert len(t_in) == K.N_IN
    t_in = np.sort(np.array([float(x) for x in t_in]))
    if s0["ttv"] is not None:
        # cadence j belongs to transit j % 3: moved there by that bin's shift (the fixture evaluates at t - shift)
        edges, shift = ttv_tables(s0, recs[0])
        t_in = np.sort(t_in + shift[np.arange(K.N_IN) % 3])
        assert np.array_equal(np.sort(np.searchsorted(edges, t_in)), np.sort(np.arange(K.N_IN) % 3))
    # t_out: a spread of times from 0.7 to 4 durations off each event, and half an orbit away
    cand = []
    for con in cons:
        t1, _, _, t4, tc = con
        dur = t4 - t1
        for k in range(1, 13):
            cand.append(tc + dur * (mp.mpf("0.7") + mp.mpf("0.3") * k) * (1 if k % 2 else -1))
    period = 2 * mp.pi / qs[0]["n"]
    cand += [cons[0][4] + period * mp.mpf(x) for x in ("0.5", "0.47", "0.53", "0.25", "-0.25", "0.4", "-0.4", "0.6")]
    t_out = []
    for j, x in enumerate(cand):
        x = float(x)
        warped = x
        if s0["ttv"] is not None:
            x = x + shift[j % 3]
            warped = mp.mpf(x) - mp.mpf(shift[int(np.searchsorted(edges, x))])
        if all(sample_is_out(warped, s0, q) for q in qs):
            t_out.append(x)
        if len(t_out) == K.N_OUT:
            break
    assert len(t_out) == K.N_OUT, (s0["name"], len(t_out))
    return t_in, np.array(t_out)


def stencil_of(s):
    if s["stencil"] is None:
        return None, np.zeros(0), np.zeros(0)
    texp, oversample, order = s["stencil"]
    dt, w = L.stencil(oversample, order)
    return float(texp), np.array([float(x) for x in dt]), np.array([float(x) for x in w])


def sample_is_out(t, s, q):
    """every sub-exposure of a cadence at t is verified to have flux 0 with room to spare"""
    texp, sdt, _ = stencil_of(s)
    sub = [mp.mpf(t)] if texp is None else [mp.mpf(t) + mp.mpf(texp) * mp.mpf(d) for d in sdt]
    for x in sub:
        for sigma in ((1, -1) if s["sbr"] is not None else (1,)):
            b, front = b_and_side(x, q, sigma)
            clear = b > 1 + q["ror"] + mp.mpf("1e-3")
            if not (clear or (not front and s["sbr"] is None)):
                return False
    return True


def ttv_tables(s, rec):
    """(edges [2], shift [3]) of a timing-variation entry: three transits, bin k's transit at t0 + k period + ttv[k]
    (include/exoplanet_amd.h: shift = transit time of the bin minus the record's t0; edges = midpoints)"""
    period, t0 = rec[P_PERIOD], rec[P_T0]
    shift = np.array([k * period + d for k, d in enumerate(s["ttv"])])
    tt = t0 + shift
    return 0.5 * (tt[1:] + tt[:-1]), shift


# ------------------------------------------------------------------------------------------------------------------------
# one cadence of one entry
# ------------------------------------------------------------------------------------------------------------------------
def cadence(arg):
    mp.mp.dps = DPS
    rec, c, secondary, grad, t, texp, sdt, sw, shift = arg
    q = mp_record(rec)
    cm = [mp.mpf(v) for v in c]
    t = mp.mpf(t) - mp.mpf(shift)
    F, dF, dc = L.record_cadence(t, q, cm, secondary, texp, sdt, sw, grad=bool(grad), light_delay=rec[P_CLIGHT] != 0)
    b = min(b_and_side(t, q, sigma)[0] for sigma in ((1, -1) if secondary else (1,)))
    if not grad:
        return float(F), [0.0] * 11, [0.0] * 6, float(b)
    return float(F), [float(v) for v in dF], [float(v) for v in dc], float(b)


def save(path, arrays):
    """an .npz whose bytes depend on the arrays alone (numpy.savez stamps every member with the time of writing)"""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    K = table()
    S = len(K.SYSTEMS)
    recs, cs = zip(*(build_record(s) for s in K.SYSTEMS))
    t_in = np.zeros((S, K.N_IN))
    t_out = np.zeros((S, K.N_OUT))
    for label, idx in K.units():
        a, b = times_of([K.SYSTEMS[i] for i in idx], [recs[i] for i in idx], K)
        t_in[idx], t_out[idx] = a, b
    texp = np.zeros(S)
    n_sub = np.zeros(S, dtype=np.int64)
    sdt, sw = np.zeros((S, K.N_SUB_MAX)), np.zeros((S, K.N_SUB_MAX))
    ttv_n = np.zeros(S, dtype=np.int64)
    ttv_edges, ttv_shift = np.zeros((S, 2)), np.zeros((S, 3))
    jobs = []
    for i, s in enumerate(K.SYSTEMS):
        te, d, w = stencil_of(s)
        if te is not None:
            texp[i], n_sub[i] = te, d.size
            sdt[i, :d.size], sw[i, :d.size] = d, w
        if s["ttv"] is not None:
            ttv_n[i] = 3
            ttv_edges[i], ttv_shift[i] = ttv_tables(s, recs[i])
        for t in t_in[i]:
            sh = ttv_shift[i][np.searchsorted(ttv_edges[i], t)] if ttv_n[i] else 0.0
            jobs.append((recs[i], cs[i], s["sbr"] is not None, s["grad"], t, te, d, w, sh))
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(cadence, jobs, chunksize=2)
        ujobs = [(K.user_vector(s), s["ecc"] is None, s["sbr"] is not None, s["u"]) for s in K.SYSTEMS]
        ujobs += [(K.user_vector(s), False, False, s["u"]) for s in K.PACK_ONLY]
        ujobs += [(K.user_vector(s), False, True, s["u2"]) for s in K.SYSTEMS if s["sbr"] is not None]
        ures = pool.map(user_jacobian, ujobs, chunksize=1)
    flux = np.array([r[0] for r in res]).reshape(S, K.N_IN)
    jac_rec = np.array([r[1] for r in res]).reshape(S, K.N_IN, 11)
    jac_c = np.array([r[2] for r in res]).reshape(S, K.N_IN, 6)
    b_in = np.array([r[3] for r in res]).reshape(S, K.N_IN)
    # user level: the Jacobian of the packing, for the entries a user-level call can express (zeros elsewhere)
    cols = list(K.REC_COLS)
    user_in = np.array([K.user_vector(s) for s in K.SYSTEMS])
    user_u = np.array([list(s["u"]) + list(s["u2"] or (0.0, 0.0)) for s in K.SYSTEMS])
    jac_user, jac_cu = np.zeros((S, 11, 10)), np.zeros((S, 6, 4))
    sec = iter(ures[S + len(K.PACK_ONLY):])
    for i, s in enumerate(K.SYSTEMS):
        if not K.user_ok(s):
            continue
        rec_u, jac_user[i], jac_cu[i, :3, :2] = ures[i]
        if s["sbr"] is not None:
            jac_cu[i, 3:, 2:] = next(sec)[2]
        # the record the fixture's flux belongs to IS this function of the inputs, rounded once (light speed: only where used)
        keep = [j for j in range(11) if not (j == 10 and not s["light_delay"])]
        assert np.array_equal(rec_u[keep], recs[i][cols][keep]), s["name"]
    pk = ures[S:S + len(K.PACK_ONLY)]
    # two of the three planets of a group are on the disk at once in some cadence
    for label, idx in K.units():
        if len(idx) > 1:
            both = [(flux[a] < 0) & (flux[b] < 0) for a in idx for b in idx if a < b]
            assert max(int(x.sum()) for x in both) >= 2, label
    for i, s in enumerate(K.SYSTEMS):
        ror = recs[i][P_ROR]
        assert flux[i].min() < -1e-4, (s["name"], flux[i].min())
        limb = np.abs(b_in[i] - 1) < ror
        if s["sbr"] is None:
            warped = t_in[i] - (ttv_shift[i][np.searchsorted(ttv_edges[i], t_in[i])] if ttv_n[i] else 0.0)
            before = warped < recs[i][P_T0]
            assert (limb & before).sum() >= 2 and (limb & ~before).sum() >= 2, (s["name"], int(limb.sum()))
        else:           # two limb cadences on either side of both events
            assert limb.sum() >= 8, (s["name"], int(limb.sum()))
    out = dict(rec=np.array(recs), c=np.array(cs), secondary=np.array([float(s["sbr"] is not None) for s in K.SYSTEMS]),
               grad=np.array([float(s["grad"]) for s in K.SYSTEMS]),
               group=np.array([-1.0 if s["group"] is None else float(s["group"]) for s in K.SYSTEMS]),
               user_in=user_in, user_u=user_u, jac_user=jac_user, jac_cu=jac_cu,
               pk_in=np.array([K.user_vector(s) for s in K.PACK_ONLY]), pk_u=np.array([s["u"] for s in K.PACK_ONLY]),
               pk_rec=np.array([r[0] for r in pk]), pk_jac=np.array([r[1] for r in pk]),
               texp=texp, n_sub=n_sub, sdt=sdt, sw=sw, ttv_n=ttv_n, ttv_edges=ttv_edges, ttv_shift=ttv_shift, t_in=t_in, t_out=t_out, flux=flux, jac_rec=jac_rec, jac_c=jac_c, b_in=b_in)
    path = os.path.join(ROOT, "tests", "golden", "lightcurve_mp.npz")
    save(path, out)
    print(path, os.path.getsize(path), "bytes;", S, "entries x", K.N_IN, "cadences")
    for i, s in enumerate(K.SYSTEMS):
        print(f"  {i:2d} {s['name']:28s} e={recs[i][P_ECC]:.4g} cos i={recs[i][P_COSI]:.3g} a/R={recs[i][P_AOR]:.4g} "
              f"min flux={flux[i].min():.3g} limb cadences={int((np.abs(b_in[i] - 1) < recs[i][P_ROR]).sum())}")


if __name__ == "__main__":
    main()

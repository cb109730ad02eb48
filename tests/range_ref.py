"""Loop-level restatement of rules HL1..HL6 with Python floats and `math`:
each (month, asset)'s Parkinson, Corwin-Schultz and Abdi-Ranaldo sums from the daily high, low and
close panels, and the window model on them.  A helper for the tests, not a test file and not part
of the product.  One asset at a time, its days in order; every operation is one IEEE fp64
operation (Python floats), so each sum is sequential in the stated order and nothing is fused.

  HL1  row d is ranged iff H, L, C are not NaN (the ABSENT payload is a NaN), L > 0, H >= L and
       L <= C <= H; any other row is skipped and changes no state
  HL2  h = log H, l = log L, c = log C, u = h - l, eta = (h + l) * 0.5; Parkinson term u * u
  HL3  d' = the previous ranged row; (d', d) is a pair iff d - d' <= max_gap, booked in d's month;
       a run that starts at month m0 > 0 finds d' among the max_gap rows before its first row
  HL4  s = L_d > C_d' ? L_d - C_d' : (H_d < C_d' ? H_d - C_d' : 0.0); H* = H_d - s, L* = L_d - s,
       h* = log H*, l* = log L*; beta = u_d' u_d' + (h* - l*)(h* - l*);
       hh = H_d' >= H* ? h_d' : h*, ll = L_d' <= L* ? l_d' : l*, gamma = (hh - ll)(hh - ll);
       k = 3.0 - 2.0 sqrt(2.0); alpha = (sqrt(2.0 beta) - sqrt(beta)) / k - sqrt(gamma / k);
       e = exp(alpha); S = 2.0 (e - 1.0) / (1.0 + e); the pair adds S < 0 ? 0.0 : S; a NaN S
       (L* <= 0) adds nothing and is not counted in NCS
       Abdi-Ranaldo term (c_d' - eta_d') * (c_d' - eta_d)
  HL5  NRG ranged days, NPR pairs, NCS pairs with S not NaN, SPK, SCS, SAR the sums
  HL6  over months j = t-Wm+1 .. t (t-Wm+1 >= 0), each HL5 value added oldest first from zero:
       PKVOL = sqrt(spk / (c4 * nrg))            iff nrg >= min_obs, c4 = 4 ln 2
       CSSPR = scs / ncs                         iff ncs >= min_obs
       ARSPR = m > 0 ? 2.0 * sqrt(m) : 0.0, m = sar / npr   iff npr >= min_obs
       NOBS  = npr (0 before a whole window)

Beside each float sum range_sums returns the scale the device's sum is compared on (the libms
differ, and h - l and c - eta cancel): SPK its own value, SAR the sum of |term|, SCS the sum of
(sqrt(2 beta) + sqrt(beta)) / k + sqrt(gamma / k), the magnitudes that cancel in alpha.
"""
import math

import numpy as np

COUNTS = ("NRG", "NPR", "NCS")
FSUMS = ("SPK", "SCS", "SAR")
SUMS = COUNTS + FSUMS
SCALES = ("SPK_scale", "SCS_scale", "SAR_scale")
K_CS = 3.0 - 2.0 * math.sqrt(2.0)
C4 = 4.0 * math.log(2.0)
NAN = float("nan")


def _log(x):
    """log with the IEEE edge values instead of exceptions."""
    if x > 0.0:
        return math.log(x)
    return -math.inf if x == 0.0 else NAN


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN       # (NaN compares false)


def _exp(x):
    if x != x:
        return NAN
    return math.exp(x) if x < 709.0 else math.inf


def ranged(H, L, C):
    """HL1 (every comparison is false on a NaN)."""
    return L > 0.0 and H >= L and L <= C and C <= H


def cs_pair(Hp, Lp, Cp, H, L):
    """HL4 -> (S, scale) of the pair (d', d)."""
    hp, lp = _log(Hp), _log(Lp)
    h, l = _log(H), _log(L)
    s = L - Cp if L > Cp else (H - Cp if H < Cp else 0.0)
    Hs, Ls = H - s, L - s
    hs, ls = (h, l) if s == 0.0 else (_log(Hs), _log(Ls))
    up, us = hp - lp, hs - ls
    beta = up * up + us * us
    hh = hp if Hp >= Hs else hs
    ll = lp if Lp <= Ls else ls
    gamma = (hh - ll) * (hh - ll)
    a, b, g = _sqrt(2.0 * beta), _sqrt(beta), _sqrt(gamma / K_CS)
    alpha = (a - b) / K_CS - g
    e = _exp(alpha)
    S = 2.0 * (e - 1.0) / (1.0 + e)
    return S, (a + b) / K_CS + g


def _clip(d, lo, hi):
    return lo if d < lo else (hi if d > hi else d)


def range_sums(H, L, C, month_start, max_gap=1, m0=0, m1=None):
    """HL1..HL5 for months [m0, m1) -> dict of SUMS and SCALES, each [m1 - m0][N] (COUNTS int32)."""
    T_d, N = H.shape
    T_m = len(month_start) - 1
    m1 = T_m if m1 is None else m1
    out = {k: np.zeros((m1 - m0, N), dtype=np.int32) for k in COUNTS}
    out.update({k: np.zeros((m1 - m0, N)) for k in FSUMS + SCALES})
    dA = _clip(int(month_start[m0]), 0, T_d)
    dB = _clip(int(month_start[m1]), dA, T_d)
    ends = [_clip(int(month_start[m + 1]), dA, dB) for m in range(m0, m1)]
    ends[-1] = dB
    for a in range(N):
        Hc, Lc, Cc = H[:, a].tolist(), L[:, a].tolist(), C[:, a].tolist()
        prev = None                      # (row, H, L, C) of the latest ranged row
        for g in range(1, max_gap + 1):  # the lead-in
            d = dA - g
            if d < 0:
                break
            if ranged(Hc[d], Lc[d], Cc[d]):
                prev = (d, Hc[d], Lc[d], Cc[d])
                break
        d = dA
        for i, end in enumerate(ends):
            nrg = npr = ncs = 0
            spk = scs = sar = 0.0
            scs_s = sar_s = 0.0
            while d < end:
                Hd, Ld, Cd = Hc[d], Lc[d], Cc[d]
                if ranged(Hd, Ld, Cd):
                    h, l, c = _log(Hd), _log(Ld), _log(Cd)
                    u = h - l
                    eta = (h + l) * 0.5
                    nrg += 1
                    spk = spk + u * u
                    if prev is not None and d - prev[0] <= max_gap:
                        _, Hp, Lp, Cp = prev
                        npr += 1
                        S, sc = cs_pair(Hp, Lp, Cp, Hd, Ld)
                        if S == S:
                            ncs += 1
                            scs = scs + (0.0 if S < 0.0 else S)
                            scs_s = scs_s + sc
                        hp, lp, cp = _log(Hp), _log(Lp), _log(Cp)
                        etap = (hp + lp) * 0.5
                        term = (cp - etap) * (cp - eta)
                        sar = sar + term
                        sar_s = sar_s + abs(term)
                    prev = (d, Hd, Ld, Cd)
                d += 1
            out["NRG"][i, a], out["NPR"][i, a], out["NCS"][i, a] = nrg, npr, ncs
            out["SPK"][i, a], out["SCS"][i, a], out["SAR"][i, a] = spk, scs, sar
            out["SPK_scale"][i, a], out["SCS_scale"][i, a], out["SAR_scale"][i, a] = spk, scs_s, sar_s
    return out


MODEL = ("PKVOL", "CSSPR", "ARSPR", "NOBS")


def range_model(sums, Wm=1, min_obs=None, c4=C4):
    """HL6 -> dict of MODEL, each [T_m][N] (NOBS int32)."""
    T_m, N = sums["SPK"].shape
    min_obs = 15 * Wm if min_obs is None else min_obs
    out = {k: np.full((T_m, N), np.nan) for k in MODEL[:3]}
    out["NOBS"] = np.zeros((T_m, N), dtype=np.int32)
    cols = {k: np.asarray(sums[k]).tolist() for k in SUMS}
    for t in range(Wm - 1, T_m):
        for a in range(N):
            nrg = npr = ncs = 0
            spk = scs = sar = 0.0
            for j in range(t - Wm + 1, t + 1):
                nrg += cols["NRG"][j][a]
                npr += cols["NPR"][j][a]
                ncs += cols["NCS"][j][a]
                spk = spk + cols["SPK"][j][a]
                scs = scs + cols["SCS"][j][a]
                sar = sar + cols["SAR"][j][a]
            if nrg >= min_obs:
                out["PKVOL"][t, a] = _sqrt(spk / (c4 * float(nrg)))
            if ncs >= min_obs:
                out["CSSPR"][t, a] = scs / float(ncs)
            if npr >= min_obs:
                m = sar / float(npr)
                out["ARSPR"][t, a] = 2.0 * _sqrt(m) if m > 0.0 else 0.0
            out["NOBS"][t, a] = npr
    return out

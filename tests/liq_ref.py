"""Loop-level NumPy restatement of rules Q1..Q3: each (month, asset)'s day
counts, volume, dollar volume and Amihud sums from the daily price and volume panels, and the
window model on them -- ILLIQ, dollar average daily volume, turnover, and the shares of zero-return
and zero-volume days.  A helper for the tests, not a test file and not part of the product.  Loops
run over days and months; every step is elementwise over the assets, so each asset's sums are
sequential in the stated order and no operation is fused.

  Q1  v = V with NaN as 0.0; a day is priced when P is not NaN (the ABSENT payload is a NaN);
      dv = P * v on priced days; r = rule V1's return (dailymkt_ref.daily_ret) with max_gap.
      Volume on an unpriced day is ignored.
  Q2  per (month t, asset), days d of [month_start[t], month_start[t+1]) in day order from 0:
      priced day:                      NP += 1, SV += v, SDV += dv, NZV += (v == 0)
      return day (r not NaN):          ND += 1, NZR += (r == 0)
      Amihud day (r not NaN, dv > 0):  NA += 1, SIL += |r| / dv
  Q3  over months j = t-Wm+1 .. t (t-Wm+1 >= 0), each Q2 value added oldest first from zero:
      ILLIQ = (SIL / na) * scale  iff na >= min_obs
      DVOL  = SDV / np            iff np >= min_obs
      TURN  = (SV / np) / SH[t]   iff np >= min_obs and SH[t] > 0
      ZRET  = nzr / nd            iff nd >= min_obs
      ZVOL  = nzv / np            iff np >= min_obs
      NOBS  = na (0 before a whole window)
"""
import numpy as np

from dailymkt_ref import daily_ret

COUNTS = ("NP", "ND", "NA", "NZR", "NZV")
FSUMS = ("SV", "SDV", "SIL")
SUMS = COUNTS + FSUMS


def liq_sums(P, V, month_start, max_gap=10):
    """Q1, Q2 -> dict of SUMS, each [T_m][N] (COUNTS int32), plus R [T_d][N]."""
    T_d, N = P.shape
    T_m = len(month_start) - 1
    R = daily_ret(P, max_gap)
    out = {k: np.zeros((T_m, N), dtype=np.int32) for k in COUNTS}
    out.update({k: np.zeros((T_m, N)) for k in FSUMS})
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T_m):
            npd, nd, na, nzr, nzv = (np.zeros(N, dtype=np.int32) for _ in range(5))
            sv, sdv, sil = (np.zeros(N) for _ in range(3))
            for d in range(int(month_start[t]), int(month_start[t + 1])):
                x, r = P[d], R[d]
                v = np.where(np.isnan(V[d]), 0.0, V[d])
                priced = ~np.isnan(x)
                ret = ~np.isnan(r)
                dv = x * v
                ami = ret & (dv > 0.0)
                q = np.abs(r) / dv
                npd = npd + priced
                sv = np.where(priced, sv + v, sv)
                sdv = np.where(priced, sdv + dv, sdv)
                nzv = nzv + (priced & (v == 0.0))
                nd = nd + ret
                nzr = nzr + (ret & (r == 0.0))
                na = na + ami
                sil = np.where(ami, sil + q, sil)
            out["NP"][t], out["ND"][t], out["NA"][t] = npd, nd, na
            out["NZR"][t], out["NZV"][t] = nzr, nzv
            out["SV"][t], out["SDV"][t], out["SIL"][t] = sv, sdv, sil
    out["R"] = R
    return out


MODEL = ("ILLIQ", "DVOL", "TURN", "ZRET", "ZVOL", "NOBS")


def liq_model(sums, Wm=12, min_obs=None, scale=1e6, SH=None):
    """Q3 -> dict of MODEL, each [T_m][N] (NOBS int32); TURN is all NaN without SH."""
    T_m, N = sums["SDV"].shape
    min_obs = 15 * Wm if min_obs is None else min_obs
    out = {k: np.full((T_m, N), np.nan) for k in MODEL[:5]}
    out["NOBS"] = np.zeros((T_m, N), dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(Wm - 1, T_m):
            npd, nd, na, nzr, nzv = (np.zeros(N, dtype=np.int64) for _ in range(5))
            sv, sdv, sil = (np.zeros(N) for _ in range(3))
            for j in range(t - Wm + 1, t + 1):
                npd = npd + sums["NP"][j]
                nd = nd + sums["ND"][j]
                na = na + sums["NA"][j]
                nzr = nzr + sums["NZR"][j]
                nzv = nzv + sums["NZV"][j]
                sv = sv + sums["SV"][j]
                sdv = sdv + sums["SDV"][j]
                sil = sil + sums["SIL"][j]
            naf, npf, ndf = (c.astype(np.float64) for c in (na, npd, nd))
            out["ILLIQ"][t] = np.where(na >= min_obs, (sil / naf) * scale, np.nan)
            out["DVOL"][t] = np.where(npd >= min_obs, sdv / npf, np.nan)
            if SH is not None:
                adv = sv / npf
                out["TURN"][t] = np.where((npd >= min_obs) & (SH[t] > 0.0), adv / SH[t], np.nan)
            out["ZRET"][t] = np.where(nd >= min_obs, nzr.astype(np.float64) / ndf, np.nan)
            out["ZVOL"][t] = np.where(npd >= min_obs, nzv.astype(np.float64) / npf, np.nan)
            out["NOBS"][t] = na
    return out

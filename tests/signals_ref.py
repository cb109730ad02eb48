"""Loop-level NumPy restatement of rules D1..D6: the 52-week high, the
realised daily volatility and volatility-scaled momentum, from every day row of the panel.  A
helper for the tests, not a test file and not part of the product.  Loops run over days and
months; every step is elementwise over the assets, so each asset's sums are sequential in the
stated order and no operation is fused.

  D1  per (month t, asset), rows [month_start[t], month_start[t+1]); priced = not NaN (the ABSENT
      payload is a NaN):  PM last priced price (NaN: rows but no price; ABSENT: no row), P1 first
      priced price, HI their maximum, and over consecutive priced rows d' < d of the month
      r = P[d] / P[d'] - 1, SSW += r * r, NDW += 1
  D2  q = last priced PM of the months before t; where P1[t] is priced and q is not NaN,
      r0 = P1[t] / q - 1, SS = SSW + r0 * r0, ND = NDW + 1; first = first priced month
  D3  H52[t] = PM[t] / max HI[t-Jh+1 .. t]   iff PM[t] priced, t-Jh+1 >= 0, first <= t-Jh+1
  D4  RV[t] = sqrt(sum SS / sum ND) over t-Jv+1 .. t, oldest first   iff t-Jv+1 >= 0,
      first <= t-Jv+1, sum ND >= min_obs
  D5  MS[t] = M[t] / RV[t]   iff neither is NaN and RV[t] > 0
  D6  next return of a signal S: ranked = (PM not ABSENT) and (S not NaN); the price is
      forward-filled within the ranked subset; a ranked row's return is settled by the asset's
      next present row; the last ranked row's is NaN
"""
import numpy as np

from oracle.csmom_oracle import absent_like, absent_scalar, is_absent


def month_stats(P, month_start):
    """D1 -> dict(PM, P1, HI, SSW, NDW), each [T_m][N] (NDW int32)."""
    T_d, N = P.shape
    T_m = len(month_start) - 1
    PM = absent_like((T_m, N))
    P1 = np.full((T_m, N), np.nan)
    HI = np.full((T_m, N), np.nan)
    SSW = np.zeros((T_m, N))
    NDW = np.zeros((T_m, N), dtype=np.int32)
    here = ~is_absent(P)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T_m):
            last = np.full(N, np.nan)
            p1 = np.full(N, np.nan)
            hi = np.full(N, np.nan)
            ss = np.zeros(N)
            nd = np.zeros(N, dtype=np.int32)
            anyp = np.zeros(N, dtype=bool)
            for d in range(int(month_start[t]), int(month_start[t + 1])):
                x = P[d]
                ok = ~np.isnan(x)
                have = ok & ~np.isnan(last)
                r = x / last - 1.0
                sq = r * r
                ss = np.where(have, ss + sq, ss)
                nd = nd + have
                hi = np.where(ok & (np.isnan(hi) | (x > hi)), x, hi)
                p1 = np.where(ok & np.isnan(p1), x, p1)
                last = np.where(ok, x, last)
                anyp |= here[d]
            PM[t] = np.where(anyp, last, absent_scalar())
            P1[t], HI[t], SSW[t], NDW[t] = p1, hi, ss, nd
    return dict(PM=PM, P1=P1, HI=HI, SSW=SSW, NDW=NDW)


def next_ret(PM, S):
    """D6 -> NR [T_m][N]."""
    T_m, N = PM.shape
    NR = np.full((T_m, N), np.nan)
    psff = np.full(N, np.nan)
    prev = np.full(N, -1, dtype=np.int64)
    cols = np.arange(N)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T_m):
            pres = ~is_absent(PM[t])
            ranked = pres & ~np.isnan(S[t])
            ps_new = np.where(np.isnan(PM[t]), psff, PM[t])
            nr = ps_new / psff - 1.0
            pend = pres & (prev >= 0)
            NR[prev[pend], cols[pend]] = nr[pend]
            psff = np.where(ranked, ps_new, psff)
            prev = np.where(pres, np.where(ranked, t, -1), prev)
    return NR


def window_signals(PM, P1, HI, SSW, NDW, M=None, Jh=12, Jv=12, min_obs=None):
    """D2..D6 -> dict(SS, ND, H52, RV, MS, NR_H52, NR_MS); MS / NR_MS None without M."""
    T_m, N = PM.shape
    min_obs = 10 * Jv if min_obs is None else min_obs
    SS = np.zeros((T_m, N))
    ND = np.zeros((T_m, N), dtype=np.int32)
    H52 = np.full((T_m, N), np.nan)
    RV = np.full((T_m, N), np.nan)
    q = np.full(N, np.nan)
    first = np.full(N, T_m, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T_m):
            priced = ~np.isnan(PM[t])
            first = np.where(priced & (first == T_m), t, first)
            stitch = ~np.isnan(P1[t]) & ~np.isnan(q)
            r0 = P1[t] / q - 1.0
            sq = r0 * r0
            SS[t] = np.where(stitch, SSW[t] + sq, SSW[t])
            ND[t] = NDW[t] + stitch
            if t - Jh + 1 >= 0:
                hmax = np.full(N, np.nan)
                for j in range(t - Jh + 1, t + 1):
                    h = HI[j]
                    hmax = np.where(~np.isnan(h) & (np.isnan(hmax) | (h > hmax)), h, hmax)
                ok = priced & (first <= t - Jh + 1)
                H52[t] = np.where(ok, PM[t] / hmax, np.nan)
            if t - Jv + 1 >= 0:
                s = np.zeros(N)
                n = np.zeros(N, dtype=np.int64)
                for j in range(t - Jv + 1, t + 1):
                    s = s + SS[j]
                    n = n + ND[j]
                ok = (first <= t - Jv + 1) & (n >= min_obs)
                RV[t] = np.where(ok, np.sqrt(s / n.astype(np.float64)), np.nan)
            q = np.where(priced, PM[t], q)
        MS = None
        if M is not None:
            MS = np.where(~np.isnan(M) & (RV > 0), M / RV, np.nan)
    return dict(SS=SS, ND=ND, H52=H52, RV=RV, MS=MS, NR_H52=next_ret(PM, H52),
                NR_MS=None if MS is None else next_ret(PM, MS))


def signals(P, month_start, M=None, Jh=12, Jv=12, min_obs=None):
    """D1..D6 end to end: month_stats' and window_signals' outputs in one dict."""
    st = month_stats(P, month_start)
    out = dict(st)
    out.update(window_signals(st["PM"], st["P1"], st["HI"], st["SSW"], st["NDW"], M, Jh, Jv,
                              min_obs))
    return out

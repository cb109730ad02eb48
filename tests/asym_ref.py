"""Loop-level NumPy restatement of rules AS1..AS3: each (month, asset)'s
return days by the sign of the return with their squared returns, its market-model sums over the
days on one side of a daily series, and the window model on them -- information discreteness, the
signed jump variation RSJ, the downside semi-volatility and the side beta.  A helper for the tests,
not a test file and not part of the product.  Loops run over days and months; every step is
elementwise over the assets, so each asset's sums are sequential in the stated order and no
operation is fused.

  AS1 r = rule V1's return (dailymkt_ref.daily_ret) with max_gap; f = FD[d], which may be NaN;
      side -1: the side days have f < 0; side +1: f > 0.
  AS2 per (month t, asset), days d of [month_start[t], month_start[t+1]) in day order from zero,
      rr = r * r:
      return day (r not NaN):                  ND += 1
      r > 0:                                   NUP += 1, SUP += rr
      r < 0:                                   NDN += 1, SDN += rr     (r == 0: ND only)
      side day (r, f not NaN, f on the side):  NB += 1, BR += r, BF += f, BFF += f * f, BRF += r * f
      Without FD the five side panels are None.
  AS3 over months j = t-skip-Wm+1 .. t-skip (t-skip-Wm+1 >= 0), each AS2 value added oldest first
      from zero:
      ID     = q if M[t] > 0, -q if M[t] < 0, 0.0 if M[t] == 0, NaN if M[t] is NaN,
               q = (ndn - nup) / nd          iff nd >= min_obs
      RSJ    = (sup - sdn) / (sup + sdn)     iff nd >= min_obs and sup + sdn > 0
      DSVOL  = sqrt(sdn / nd)                iff nd >= min_obs
      DNBETA = crf / cff, mf = bf / nb, cff = bff - bf * mf, crf = brf - br * mf
                                             iff nb >= min_side and cff > 0
      NOBS = nd, NSIDE = nb (0 before a whole window)
"""
import numpy as np

from dailymkt_ref import daily_ret

COUNTS = ("ND", "NUP", "NDN")
FSUMS = ("SUP", "SDN")
SIDE_COUNTS = ("NB",)
SIDE_FSUMS = ("BR", "BF", "BFF", "BRF")
SIDE = SIDE_COUNTS + SIDE_FSUMS
SUMS = COUNTS + FSUMS + SIDE           # the C ABI's order


def asym_sums(P, month_start, FD=None, side=-1, max_gap=10):
    """AS1, AS2 -> dict of SUMS, each [T_m][N] (counts int32; SIDE None without FD), plus R."""
    assert side in (-1, 1)
    T_d, N = P.shape
    T_m = len(month_start) - 1
    R = daily_ret(P, max_gap)
    hasf = FD is not None
    out = {k: np.zeros((T_m, N), dtype=np.int32) for k in COUNTS + SIDE_COUNTS}
    out.update({k: np.zeros((T_m, N)) for k in FSUMS + SIDE_FSUMS})
    with np.errstate(invalid="ignore"):
        for t in range(T_m):
            nd, nup, ndn, nb = (np.zeros(N, dtype=np.int32) for _ in range(4))
            sup, sdn, br, bf, bff, brf = (np.zeros(N) for _ in range(6))
            for d in range(int(month_start[t]), int(month_start[t + 1])):
                r = R[d]
                ret = ~np.isnan(r)
                up = r > 0.0
                dn = r < 0.0
                rr = r * r
                nd = nd + ret
                nup = nup + up
                sup = np.where(up, sup + rr, sup)
                ndn = ndn + dn
                sdn = np.where(dn, sdn + rr, sdn)
                if hasf:
                    f = np.full(N, FD[d])
                    on = (f < 0.0) if side < 0 else (f > 0.0)      # a NaN f is on neither side
                    b = ret & on
                    ff = f * f
                    rf = r * f
                    nb = nb + b
                    br = np.where(b, br + r, br)
                    bf = np.where(b, bf + f, bf)
                    bff = np.where(b, bff + ff, bff)
                    brf = np.where(b, brf + rf, brf)
            out["ND"][t], out["NUP"][t], out["NDN"][t] = nd, nup, ndn
            out["SUP"][t], out["SDN"][t] = sup, sdn
            out["NB"][t], out["BR"][t], out["BF"][t] = nb, br, bf
            out["BFF"][t], out["BRF"][t] = bff, brf
    if not hasf:
        for k in SIDE:
            out[k] = None
    out["R"] = R
    return out


MODEL = ("ID", "RSJ", "DSVOL", "DNBETA", "NOBS", "NSIDE")


def asym_model(sums, Wm=12, skip=0, M=None, min_obs=None, min_side=None):
    """AS3 -> dict of MODEL, each [T_m][N] (NOBS, NSIDE int32); ID is all NaN without M, DNBETA
    all NaN and NSIDE all 0 without the side panels."""
    T_m, N = sums["SUP"].shape
    min_obs = 15 * Wm if min_obs is None else min_obs
    min_side = max(2, 5 * Wm) if min_side is None else min_side
    hasf = sums["NB"] is not None
    out = {k: np.full((T_m, N), np.nan) for k in MODEL[:4]}
    out["NOBS"] = np.zeros((T_m, N), dtype=np.int32)
    out["NSIDE"] = np.zeros((T_m, N), dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(skip + Wm - 1, T_m):
            nd, nup, ndn, nb = (np.zeros(N, dtype=np.int64) for _ in range(4))
            sup, sdn, br, bf, bff, brf = (np.zeros(N) for _ in range(6))
            for j in range(t - skip - Wm + 1, t - skip + 1):
                nd = nd + sums["ND"][j]
                nup = nup + sums["NUP"][j]
                ndn = ndn + sums["NDN"][j]
                sup = sup + sums["SUP"][j]
                sdn = sdn + sums["SDN"][j]
                if hasf:
                    nb = nb + sums["NB"][j]
                    br = br + sums["BR"][j]
                    bf = bf + sums["BF"][j]
                    bff = bff + sums["BFF"][j]
                    brf = brf + sums["BRF"][j]
            ndf, nbf = nd.astype(np.float64), nb.astype(np.float64)
            enough = nd >= min_obs
            if M is not None:
                m = M[t]
                q = (ndn - nup).astype(np.float64) / ndf
                idv = np.where(m > 0.0, q, np.where(m < 0.0, -q, np.where(m == 0.0, 0.0, np.nan)))
                out["ID"][t] = np.where(enough, idv, np.nan)
            tot = sup + sdn
            out["RSJ"][t] = np.where(enough & (tot > 0.0), (sup - sdn) / tot, np.nan)
            out["DSVOL"][t] = np.where(enough, np.sqrt(sdn / ndf), np.nan)
            if hasf:
                mf = bf / nbf
                cff = bff - bf * mf
                crf = brf - br * mf
                out["DNBETA"][t] = np.where((nb >= min_side) & (cff > 0.0), crf / cff, np.nan)
            out["NOBS"][t] = nd
            out["NSIDE"][t] = nb
    return out

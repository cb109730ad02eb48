"""Loop-level NumPy restatement of rules B1..B6: the equal-weight market
return, each asset's market model on it (beta, alpha, idiosyncratic volatility, residual momentum)
and the next return of any signal.  A helper for the tests, not a test file and not part of the
product.  Loops run over months; every step is elementwise over the assets, so each asset's sums
are sequential in the stated order and no operation is fused.

  B1  x[t] = PM[t] / PM[t-1] - 1 where both calendar-adjacent month prices are priced (not NaN;
      the ABSENT payload is a NaN), else NaN; x[0] is NaN
  B2  NMK[t] = assets with an observation; MKT[t] = (sum of x[t]) / NMK[t] iff NMK[t] >= min_assets
      -- the sum here is math.fsum, the exact sum and not an order
  B3  over the Wb months j = t-Wb+1 .. t (t-Wb+1 >= 0), observations where x[j] and f[j] are both
      not NaN, n of them.  Oldest first: sx += x, sf += f; mx = sx / n, mf = sf / n; then
      df = f - mf, dx = x - mx, sff += df * df, sfx += df * dx.  BETA = sfx / sff,
      ALPHA = mx - BETA * mf, both iff n >= min_obs and sff > 0; NOBS = n
  B4  e[j] = x[j] - (ALPHA + BETA * f[j]); IVOL = sqrt(sum e^2 / (n - 2)) iff BETA and n >= 3
  B5  formation months j = t-skip-J+1 .. t-skip: se = sum e, me = se / J, sv = sum (e - me)^2,
      RESMOM = se / sqrt(sv / (J - 1)) iff BETA, all J months are observations, and sv > 0
  B6  the next return of a signal: signals_ref.next_ret (rule D6)
"""
import math

import numpy as np

from oracle import csmom_oracle as O
from oracle.synth_np import make_panel
from signals_ref import next_ret  # noqa: F401  (B6 is D6)

T_DAYS = 1305           # 60 whole business-day months from 2000-01-03
GAPPY = dict(late=0.2, delist=0.2, nan_day=0.01, absent_month=0.01, nan_month=0.01)
DENSE = dict(late=0, delist=0, nan_day=0, absent_month=0, nan_month=0)
# (Wb, J, skip, min_obs) of the tests
CASES = [(24, 11, 1, 18), (12, 6, 1, 10), (3, 2, 0, 3), (36, 12, 1, 24), (60, 12, 1, 40)]
_PANELS = {}


def panel(N, kind="gappy"):
    """The tests' panel of N assets x 60 months: dict(P, ms, PM), made once and left unchanged."""
    if (N, kind) not in _PANELS:
        pan = make_panel(N, T_DAYS, seed=300 + N, cents=True, with_volume=False,
                         **(DENSE if kind == "dense" else GAPPY))
        PM, _ = O.month_end(pan["P"], pan["month_start"])
        assert PM.shape == (60, N)
        _PANELS[(N, kind)] = dict(P=pan["P"], ms=pan["month_start"], PM=PM)
    return _PANELS[(N, kind)]


def month_returns(PM):
    """B1 -> X [T_m][N]."""
    T_m, N = PM.shape
    X = np.full((T_m, N), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, T_m):
            ok = ~np.isnan(PM[t]) & ~np.isnan(PM[t - 1])
            X[t] = np.where(ok, PM[t] / PM[t - 1] - 1.0, np.nan)
    return X


def market_factor(PM, min_assets=1):
    """B1, B2 -> dict(X, MKT, NMK, SABS); SABS[t] = fsum |x[t]|, what the error bound of a
    summation order is stated in."""
    X = month_returns(PM)
    T_m = X.shape[0]
    MKT = np.full(T_m, np.nan)
    NMK = np.zeros(T_m, dtype=np.int32)
    SABS = np.zeros(T_m)
    for t in range(T_m):
        v = X[t][~np.isnan(X[t])]
        NMK[t] = len(v)
        SABS[t] = math.fsum(np.abs(v))
        if len(v) >= min_assets:
            MKT[t] = math.fsum(v) / float(len(v))
    return dict(X=X, MKT=MKT, NMK=NMK, SABS=SABS)


def market_model(PM, F, Wb, J, skip, min_obs):
    """B1, B3..B5 -> dict(BETA, ALPHA, IVOL, RESMOM, NOBS), each [T_m][N] (NOBS int32)."""
    assert 2 <= Wb <= 60 and 2 <= min_obs <= Wb and J >= 2 and skip >= 0 and J + skip <= Wb
    X = month_returns(PM)
    T_m, N = X.shape
    out = {k: np.full((T_m, N), np.nan) for k in ("BETA", "ALPHA", "IVOL", "RESMOM")}
    NOBS = np.zeros((T_m, N), dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(Wb - 1, T_m):
            win = range(t - Wb + 1, t + 1)
            obs = {j: ~np.isnan(X[j]) & ~np.isnan(F[j]) for j in win}
            n = np.zeros(N, dtype=np.int64)
            sx = np.zeros(N)
            sf = np.zeros(N)
            for j in win:
                sx = np.where(obs[j], sx + X[j], sx)
                sf = np.where(obs[j], sf + F[j], sf)
                n = n + obs[j]
            nf = n.astype(np.float64)
            mx = sx / nf
            mf = sf / nf
            sff = np.zeros(N)
            sfx = np.zeros(N)
            for j in win:
                df = F[j] - mf
                dx = X[j] - mx
                p = df * df
                c = df * dx
                sff = np.where(obs[j], sff + p, sff)
                sfx = np.where(obs[j], sfx + c, sfx)
            ok = (n >= min_obs) & (sff > 0.0)
            beta = np.where(ok, sfx / sff, np.nan)
            bm = beta * mf
            alpha = np.where(ok, mx - bm, np.nan)

            def resid(j):
                bf = beta * F[j]
                return X[j] - (alpha + bf)

            se2 = np.zeros(N)
            for j in win:
                e = resid(j)
                sq = e * e
                se2 = np.where(obs[j], se2 + sq, se2)
            ivol = np.where(ok & (n >= 3), np.sqrt(se2 / (nf - 2.0)), np.nan)
            form = range(t - skip - J + 1, t - skip + 1)
            full = ok.copy()
            se = np.zeros(N)
            for j in form:
                full &= obs[j]
                se = se + resid(j)
            me = se / float(J)
            sv = np.zeros(N)
            for j in form:
                d = resid(j) - me
                sv = sv + d * d
            good = full & (sv > 0.0)
            resmom = np.where(good, se / np.sqrt(sv / float(J - 1)), np.nan)
            out["BETA"][t], out["ALPHA"][t], out["IVOL"][t], out["RESMOM"][t] = (beta, alpha, ivol,
                                                                                 resmom)
            NOBS[t] = n
    out["NOBS"] = NOBS
    return out

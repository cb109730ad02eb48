"""Loop-level NumPy restatement of rules MF1..MF7: the KF-factor rolling
models on the monthly returns (slopes, intercept, idiosyncratic volatility, R2, residual momentum)
and on the daily returns (month sums, window model).  A helper for the tests, not a test file and
not part of the product.  Loops run over months, days, window entries and the (at most four)
factors; every step is elementwise over the assets, so each asset's sums are sequential in the
stated order and no operation is fused.

  MF1  x = market_ref.month_returns (B1); an observation of the window j = t-Wb+1 .. t is a month
       with x[j] not NaN and no NaN in F[j][0 .. KF-1]; NOBS = n
  MF2  pass 1 oldest first: sx += x, sf_k += f_k; mx = sx / n, mf_k = sf_k / n.  pass 2 oldest
       first: dx = x - mx, d_k = f_k - mf_k, A_jk += d_j * d_k (j <= k), b_k += d_k * dx,
       cxx += dx * dx
  MF3  ldl_solve below
  MF4  BETA_k = g_k; ALPHA = mx, then ALPHA -= g_k * mf_k for k ascending; iff n >= min_obs and MF3
  MF5  fit = ALPHA, then fit += g_k * f_k[j]; e = x - fit; se2 = sum e^2;
       IVOL = sqrt(se2 / (n - (KF + 1))) iff n >= KF + 2; R2 = 1 - se2 / cxx iff cxx > 0;
       RESMOM = B5 on these residuals
  MF6  per (month, asset), days with r not NaN and a factor row, in day order: NO += 1, SR += r,
       SRR += r * r, SF_k += f_k, SRF_k += r * f_k, SFF_p(j,k) += f_j * f_k
  MF7  the MF6 sums added over the Wm months oldest first; mr = SR / nf, mf_k = SF_k / nf,
       A_jk = SFF_p - SF_j * mf_k, b_k = SRF_k - SR * mf_k, crr = SRR - SR * mr; DBETA = g (MF3) iff
       n >= min_obs; DALPHA = mr - sum g_k * mf_k; q = crr - sum g_k * b_k, clipped at 0;
       DIVOL = sqrt(q / (nf - (KF + 1))) iff n >= KF + 2; DR2 = 1 - q / crr iff crr > 0
"""
import numpy as np

from market_ref import month_returns

TINY = 2.0 ** -40
# The bars of the comparisons with np.linalg.lstsq, max_k |coefficient_k - lstsq_k| /
# max_k |lstsq_k| over a cell's slopes and intercept: one decade above the largest value
# test_factor_ref.py measures (its docstring), 3.836e-14 monthly and 9.169e-14 daily.
LSTSQ_TOL = dict(monthly=3.836e-13, daily=9.169e-13)


def pair(KF, j, k):
    """The packed index of the symmetric pair (j, k), j <= k."""
    assert 0 <= j <= k < KF
    return j * KF - j * (j - 1) // 2 + (k - j)


def n_pairs(KF):
    return KF * (KF + 1) // 2


def as_factors(F):
    F = np.asarray(F, dtype=np.float64)
    F = F[:, None] if F.ndim == 1 else F
    assert F.ndim == 2 and 1 <= F.shape[1] <= 4
    return F


def ldl_solve(A, b):
    """MF3 on A [n_pairs][N] (packed) and b [KF][N] -> (g [KF][N], defined [N])."""
    KF = len(b)
    N = b[0].shape[0]
    L = [[None] * KF for _ in range(KF)]
    D = [None] * KF
    ok = np.ones(N, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(KF):
            ajj = A[pair(KF, j, j)]
            d = ajj
            for p in range(j):
                sq = L[j][p] * L[j][p]
                d = d - sq * D[p]
            ok &= (ajj > 0.0) & (d > ajj * TINY)
            D[j] = d
            for i in range(j + 1, KF):
                v = A[pair(KF, j, i)]
                for p in range(j):
                    ll = L[i][p] * L[j][p]
                    v = v - ll * D[p]
                L[i][j] = v / d
        z = [None] * KF
        for j in range(KF):
            v = b[j]
            for p in range(j):
                v = v - L[j][p] * z[p]
            z[j] = v
        g = [None] * KF
        for j in range(KF - 1, -1, -1):
            v = z[j] / D[j]
            for p in range(j + 1, KF):
                v = v - L[p][j] * g[p]
            g[j] = v
    return g, ok


def factor_model(PM, F, Wb, J, skip, min_obs):
    """MF1..MF5 -> dict(BETA [KF][T_m][N], ALPHA, IVOL, RESMOM, R2 [T_m][N], NOBS int32)."""
    F = as_factors(F)
    KF = F.shape[1]
    assert KF + 1 <= Wb <= 60 and KF + 1 <= min_obs <= Wb
    assert J >= 2 and skip >= 0 and J + skip <= Wb
    X = month_returns(PM)
    T_m, N = X.shape
    assert F.shape[0] == T_m
    frow = ~np.isnan(F).any(axis=1)
    out = {k: np.full((T_m, N), np.nan) for k in ("ALPHA", "IVOL", "RESMOM", "R2")}
    out["BETA"] = np.full((KF, T_m, N), np.nan)
    NOBS = np.zeros((T_m, N), dtype=np.int32)
    NP = n_pairs(KF)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(Wb - 1, T_m):
            win = range(t - Wb + 1, t + 1)
            obs = {j: ~np.isnan(X[j]) & frow[j] for j in win}
            n = np.zeros(N, dtype=np.int64)
            sx = np.zeros(N)
            sf = [np.zeros(N) for _ in range(KF)]
            for j in win:
                sx = np.where(obs[j], sx + X[j], sx)
                for k in range(KF):
                    sf[k] = np.where(obs[j], sf[k] + F[j, k], sf[k])
                n = n + obs[j]
            nf = n.astype(np.float64)
            mx = sx / nf
            mf = [sf[k] / nf for k in range(KF)]
            A = [np.zeros(N) for _ in range(NP)]
            b = [np.zeros(N) for _ in range(KF)]
            cxx = np.zeros(N)
            for j in win:
                dx = X[j] - mx
                d = [F[j, k] - mf[k] for k in range(KF)]
                for c in range(KF):
                    for e in range(c, KF):
                        pr = d[c] * d[e]
                        p = pair(KF, c, e)
                        A[p] = np.where(obs[j], A[p] + pr, A[p])
                    pr = d[c] * dx
                    b[c] = np.where(obs[j], b[c] + pr, b[c])
                sq = dx * dx
                cxx = np.where(obs[j], cxx + sq, cxx)
            g, solved = ldl_solve(A, b)
            ok = (n >= min_obs) & solved
            beta = [np.where(ok, g[k], np.nan) for k in range(KF)]
            alpha = mx
            for k in range(KF):
                gm = beta[k] * mf[k]
                alpha = alpha - gm
            alpha = np.where(ok, alpha, np.nan)

            def resid(j):
                fit = alpha
                for k in range(KF):
                    bf = beta[k] * F[j, k]
                    fit = fit + bf
                return X[j] - fit

            se2 = np.zeros(N)
            for j in win:
                e = resid(j)
                sq = e * e
                se2 = np.where(obs[j], se2 + sq, se2)
            ivol = np.where(ok & (n >= KF + 2), np.sqrt(se2 / (nf - (KF + 1.0))), np.nan)
            r2 = np.where(ok & (cxx > 0.0), 1.0 - se2 / cxx, np.nan)
            form = range(t - skip - J + 1, t - skip + 1)
            full = ok.copy()
            se = np.zeros(N)
            for j in form:
                full &= obs[j]
                se = se + resid(j)
            me = se / float(J)
            sv = np.zeros(N)
            for j in form:
                dd = resid(j) - me
                sv = sv + dd * dd
            good = full & (sv > 0.0)
            resmom = np.where(good, se / np.sqrt(sv / float(J - 1)), np.nan)
            for k in range(KF):
                out["BETA"][k, t] = beta[k]
            out["ALPHA"][t], out["IVOL"][t], out["RESMOM"][t], out["R2"][t] = (alpha, ivol, resmom,
                                                                               r2)
            NOBS[t] = n
    out["NOBS"] = NOBS
    return out


def window_obs(PM, F, Wb, t, a):
    """The (x, factor rows) of asset a's observations in month t's window, oldest first: what an
    independent least-squares solver is given."""
    F = as_factors(F)
    X = month_returns(PM)
    js = [j for j in range(t - Wb + 1, t + 1)
          if not np.isnan(X[j, a]) and not np.isnan(F[j]).any()]
    return X[js, a], F[js]


FSUMS = ("NO", "SR", "SRR", "SF", "SRF", "SFF")


def daily_fsums(R, FD, month_start):
    """MF6 on V1's returns R [T_d][N] -> dict of FSUMS."""
    FD = as_factors(FD)
    KF = FD.shape[1]
    NP = n_pairs(KF)
    T_d, N = R.shape
    assert FD.shape[0] == T_d
    T_m = len(month_start) - 1
    out = dict(NO=np.zeros((T_m, N), dtype=np.int32), SR=np.zeros((T_m, N)),
               SRR=np.zeros((T_m, N)), SF=np.zeros((KF, T_m, N)), SRF=np.zeros((KF, T_m, N)),
               SFF=np.zeros((NP, T_m, N)))
    frow = ~np.isnan(FD).any(axis=1)
    for t in range(T_m):
        no = np.zeros(N, dtype=np.int32)
        sr, srr = np.zeros(N), np.zeros(N)
        sf = [np.zeros(N) for _ in range(KF)]
        srf = [np.zeros(N) for _ in range(KF)]
        sff = [np.zeros(N) for _ in range(NP)]
        for d in range(int(month_start[t]), int(month_start[t + 1])):
            r = R[d]
            obs = ~np.isnan(r) & frow[d]
            rr = r * r
            no = no + obs
            sr = np.where(obs, sr + r, sr)
            srr = np.where(obs, srr + rr, srr)
            for k in range(KF):
                f = np.full(N, FD[d, k])
                rf = r * f
                sf[k] = np.where(obs, sf[k] + f, sf[k])
                srf[k] = np.where(obs, srf[k] + rf, srf[k])
            for j in range(KF):
                for k in range(j, KF):
                    ff = np.full(N, FD[d, j] * FD[d, k])
                    p = pair(KF, j, k)
                    sff[p] = np.where(obs, sff[p] + ff, sff[p])
        out["NO"][t], out["SR"][t], out["SRR"][t] = no, sr, srr
        for k in range(KF):
            out["SF"][k, t], out["SRF"][k, t] = sf[k], srf[k]
        for p in range(NP):
            out["SFF"][p, t] = sff[p]
    return out


FMODEL = ("DBETA", "DALPHA", "DIVOL", "DR2", "NOBS")


def daily_fmodel(sums, Wm=1, min_obs=None):
    """MF7 -> dict of FMODEL (DBETA [KF][T_m][N], NOBS int32)."""
    KF, T_m, N = sums["SF"].shape
    NP = n_pairs(KF)
    min_obs = max(15 * Wm, KF + 1) if min_obs is None else min_obs
    assert 1 <= Wm <= 12 and min_obs >= KF + 1
    out = {k: np.full((T_m, N), np.nan) for k in ("DALPHA", "DIVOL", "DR2")}
    out["DBETA"] = np.full((KF, T_m, N), np.nan)
    out["NOBS"] = np.zeros((T_m, N), dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for t in range(Wm - 1, T_m):
            n = np.zeros(N, dtype=np.int64)
            SR, SRR = np.zeros(N), np.zeros(N)
            SF = [np.zeros(N) for _ in range(KF)]
            SRF = [np.zeros(N) for _ in range(KF)]
            SFF = [np.zeros(N) for _ in range(NP)]
            for j in range(t - Wm + 1, t + 1):
                n = n + sums["NO"][j]
                SR = SR + sums["SR"][j]
                SRR = SRR + sums["SRR"][j]
                for k in range(KF):
                    SF[k] = SF[k] + sums["SF"][k, j]
                    SRF[k] = SRF[k] + sums["SRF"][k, j]
                for p in range(NP):
                    SFF[p] = SFF[p] + sums["SFF"][p, j]
            nf = n.astype(np.float64)
            mr = SR / nf
            mf = [SF[k] / nf for k in range(KF)]
            A = [None] * NP
            b = [None] * KF
            for j in range(KF):
                for k in range(j, KF):
                    sm = SF[j] * mf[k]
                    A[pair(KF, j, k)] = SFF[pair(KF, j, k)] - sm
                sm = SR * mf[j]
                b[j] = SRF[j] - sm
            crr = SRR - SR * mr
            g, solved = ldl_solve(A, b)
            ok = (n >= min_obs) & solved
            alpha = mr
            q = crr
            for k in range(KF):
                gm = g[k] * mf[k]
                alpha = alpha - gm
                gb = g[k] * b[k]
                q = q - gb
            qp = np.where(q < 0.0, 0.0, q)
            for k in range(KF):
                out["DBETA"][k, t] = np.where(ok, g[k], np.nan)
            out["DALPHA"][t] = np.where(ok, alpha, np.nan)
            out["DIVOL"][t] = np.where(ok & (n >= KF + 2), np.sqrt(qp / (nf - (KF + 1.0))), np.nan)
            out["DR2"][t] = np.where(ok & (crr > 0.0), 1.0 - qp / crr, np.nan)
            out["NOBS"][t] = n
    return out


def seeded_factors(col0, seed, KF, sigma, nan_at=None):
    """The tests' factor panel [T][KF]: column 0 as given, columns 1.. seeded normal(0, sigma)
    series; nan_at = (row, column) sets one value NaN."""
    col0 = np.asarray(col0, dtype=np.float64)
    rng = np.random.default_rng(seed)
    extra = rng.normal(0.0, sigma, (len(col0), 3))     # always three, so KF shares columns
    F = np.concatenate([col0[:, None], extra], axis=1)[:, :KF].copy()
    if nan_at is not None and nan_at[1] < KF:
        F[nan_at] = np.nan
    return np.ascontiguousarray(F)

"""Loop-level NumPy restatement of rule E7: the daily return series of
the decile portfolios.  A helper for the tests, not a test file and not part of the product.

  pff[d][a]   last non-NaN price of column a in rows <= d (the ABSENT payload is a NaN)
  b[t][a]     pff[month_start[t+1] - 1][a]: the fill on the day before holding month t+1
  v[d][a]     pff[d][a] / b[t][a]
  C[d]        sum w v[d] / sum w over the members of the cohort (age k, bin q): L[t-k][a] == q,
              weight 1 or a finite W[t-k][a] > 0 (oracle member_weights), NR[t][a] not NaN,
              b[t][a] finite and > 0
  V_q[d]      mean of C[d] over the non-empty cohorts; 1 on the day before the month
  DR[d][q]    V_q[d] / V_q[d-1] - 1;  DLS[d] = DR[d][n_bins-1] - DR[d][0]
"""
import numpy as np

from oracle.portfolio_oracle import member_weights


def forward_fill(P):
    pff = np.full(P.shape, np.nan)
    last = np.full(P.shape[1], np.nan)
    for d in range(P.shape[0]):
        row = P[d]
        last = np.where(np.isnan(row), last, row)
        pff[d] = last
    return pff


def daily_returns(P, month_start, L, NR, n_bins=10, K=1, W=None):
    """(DR [T_d][n_bins], DLS [T_d], DCNT [T_m][K][n_bins] int32)."""
    T_d, N = P.shape
    T_m = len(month_start) - 1
    pff = forward_fill(P)
    DR = np.full((T_d, n_bins), np.nan)
    DCNT = np.zeros((T_m, K, n_bins), dtype=np.int32)
    for t in range(T_m - 1):
        d0, d1 = int(month_start[t + 1]), int(month_start[t + 2])
        b = pff[d0 - 1] if d0 >= 1 else np.full(N, np.nan)
        held = ~np.isnan(NR[t]) & np.isfinite(b) & (b > 0)
        for q in range(n_bins):
            cohorts = []
            for k in range(K):
                s = t - k
                if s < 0:
                    continue
                w = member_weights(L[s], q, None if W is None else W[s])
                use = (w > 0) & held
                DCNT[t, k, q] = use.sum()
                if use.any():
                    cohorts.append((use, w[use]))
            if not cohorts:
                continue
            prev = 1.0
            for d in range(d0, d1):
                C = [float((w * (pff[d][use] / b[use])).sum() / w.sum()) for use, w in cohorts]
                V = sum(C) / len(C)
                DR[d, q] = V / prev - 1.0
                prev = V
    DLS = DR[:, n_bins - 1] - DR[:, 0]
    return DR, DLS, DCNT


def monthly_gross(DR, month_start):
    """[T_m][n_bins]: the product of 1 + DR over the days of each month (NaN if any is NaN)."""
    T_m = len(month_start) - 1
    out = np.full((T_m, DR.shape[1]), np.nan)
    for m in range(T_m):
        out[m] = np.prod(1.0 + DR[month_start[m]:month_start[m + 1]], axis=0)
    return out

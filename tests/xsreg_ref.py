"""NumPy restatement of rules R1..R6: the per-month cross-sectional
regression (OLS, WLS, ridge on z-scores) and the time-series mean with its Newey-West
t-statistic.  A helper for the tests, not a test file and not part of the product.  The order of
every sum is the rule's: the sums over the assets are r1_sum, everything after them is scalar
Python float arithmetic (IEEE double, one rounding per operation, nothing fused).

  R1  a sum over assets: non-observations are 0.0; slice i = assets [2048 i, 2048 (i + 1)); lane
      l of 256 owns assets 2048 i + l + 256 k, k = 0..7, added in k order from 0.0; each 64
      consecutive lanes by a halving tree (h = 32..1: element j < h += element j + h); the four
      wave sums in order from 0.0; the slice sums in order from 0.0
  R2  observation: Y and every S_k not NaN (and W not NaN and > 0).  w = 1.0 without W.  n = NOBS;
      sw = sum w, sy = sum w * y, ss_k = sum w * s_k; my = sy / sw, ms_k = ss_k / sw.
      n < min_obs: the month's float outputs are NaN
  R3  dy = y - my, d_k = s_k - ms_k; C_jk = sum (w * d_j) * d_k (j <= k), c_k = sum (w * d_k) * dy,
      cyy = sum (w * dy) * dy; undefined unless every C_kk > 0 and cyy > 0
  R4  standardize: sd_k = sqrt(C_kk / sw), A0_jk = C_jk / (sd_j * sd_k), b_k = c_k / sd_k; else
      A0 = C, b = c.  A = A0 with A_kk = A0_kk + ridge
  R5  Cholesky with the pivot rule d > A_jj * 2^-40, forward, back, intercept, fit (solve below)
  R6  newey_west below
"""
import math

import numpy as np

SLICE, PER, LANES, WAVE = 2048, 8, 256, 64
MAX_K = 8
PIVOT = 2.0 ** -40


def r1_sum(V):
    """R1 over the last axis of V [..., N], whose non-observations are already 0.0 -> [...]."""
    V = np.asarray(V, dtype=np.float64)
    lead, N = V.shape[:-1], V.shape[-1]
    S = -(-N // SLICE)
    pad = np.zeros(lead + (S * SLICE,))
    pad[..., :N] = V
    a = pad.reshape(lead + (S, PER, LANES))
    lane = np.zeros(lead + (S, LANES))
    for k in range(PER):
        lane = lane + a[..., k, :]
    w = lane.reshape(lead + (S, LANES // WAVE, WAVE)).copy()
    h = WAVE // 2
    while h:
        w[..., :h] = w[..., :h] + w[..., h:2 * h]
        h //= 2
    sl = np.zeros(lead + (S,))
    for v in range(LANES // WAVE):
        sl = sl + w[..., v, 0]
    tot = np.zeros(lead)
    for i in range(S):
        tot = tot + sl[..., i]
    return tot


def solve(K, sw, my, ms, C, c, cyy, standardize, ridge):
    """R3's condition, R4 and R5 on one month's moments (Python floats; C a full symmetric K x K
    list of lists).  Returns (gamma [K + 1], R2), or None when the month is undefined."""
    if not (cyy > 0.0) or not all(C[k][k] > 0.0 for k in range(K)):
        return None
    if standardize:
        sd = [math.sqrt(C[k][k] / sw) for k in range(K)]
        A0 = [[C[j][k] / (sd[j] * sd[k]) for k in range(K)] for j in range(K)]
        b = [c[k] / sd[k] for k in range(K)]
    else:
        A0 = [row[:] for row in C]
        b = list(c)
    A = [row[:] for row in A0]
    for k in range(K):
        A[k][k] = A0[k][k] + ridge
    L = [[0.0] * K for _ in range(K)]
    for j in range(K):
        d = A[j][j]
        for p in range(j):
            d = d - L[j][p] * L[j][p]
        if not (d > A[j][j] * PIVOT):
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, K):
            v = A[i][j]
            for p in range(j):
                v = v - L[i][p] * L[j][p]
            L[i][j] = v / L[j][j]
    z = [0.0] * K
    for j in range(K):
        s = 0.0
        for p in range(j):
            s = s + L[j][p] * z[p]
        z[j] = (b[j] - s) / L[j][j]
    g = [0.0] * K
    for j in range(K - 1, -1, -1):
        s = 0.0
        for p in range(j + 1, K):
            s = s + L[p][j] * g[p]
        g[j] = (z[j] - s) / L[j][j]
    g0 = my
    if not standardize:
        for k in range(K):
            g0 = g0 - g[k] * ms[k]
    gb = 0.0
    for j in range(K):
        gb = gb + g[j] * b[j]
    gAg = 0.0
    for j in range(K):
        r = 0.0
        for k in range(K):
            r = r + A0[j][k] * g[k]
        gAg = gAg + g[j] * r
    rss = (cyy - 2.0 * gb) + gAg
    return [g0] + g, 1.0 - rss / cyy


def xs_regress(Y, S, W=None, standardize=False, ridge=0.0, min_obs=None):
    """R1..R5 -> dict(GAMMA [T_m][K + 1], R2 [T_m], NOBS [T_m] int32, MY [T_m]); MY is the month's
    weighted mean of Y (NaN below min_obs), what GAMMA[:, 0] is when standardised."""
    Y = np.asarray(Y, dtype=np.float64)
    S = [np.asarray(s, dtype=np.float64) for s in S]
    K = len(S)
    assert 1 <= K <= MAX_K and ridge >= 0.0
    min_obs = K + 2 if min_obs is None else int(min_obs)
    assert min_obs >= K + 2
    T_m, N = Y.shape
    GAMMA = np.full((T_m, K + 1), np.nan)
    R2 = np.full(T_m, np.nan)
    MY = np.full(T_m, np.nan)
    NOBS = np.zeros(T_m, dtype=np.int32)
    iu = [(j, k) for j in range(K) for k in range(j, K)]
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T_m):
            y = Y[t]
            s = [x[t] for x in S]
            obs = ~np.isnan(y)
            for x in s:
                obs &= ~np.isnan(x)
            if W is not None:
                obs &= ~np.isnan(W[t]) & (W[t] > 0.0)
                w = np.where(obs, W[t], 0.0)
            else:
                w = np.where(obs, 1.0, 0.0)
            n = int(obs.sum())
            NOBS[t] = n
            if n < min_obs:
                continue
            p1 = r1_sum(np.stack([w, np.where(obs, w * y, 0.0)]
                                 + [np.where(obs, w * x, 0.0) for x in s]))
            sw = float(p1[0])
            my = float(p1[1]) / sw
            ms = [float(p1[2 + k]) / sw for k in range(K)]
            MY[t] = my
            dy = y - my
            d = [s[k] - ms[k] for k in range(K)]
            wd = [w * d[k] for k in range(K)]
            wdy = w * dy
            rows = [wd[j] * d[k] for j, k in iu] + [wd[k] * dy for k in range(K)] + [wdy * dy]
            p2 = r1_sum(np.stack([np.where(obs, r, 0.0) for r in rows]))
            C = [[0.0] * K for _ in range(K)]
            for q, (j, k) in enumerate(iu):
                C[j][k] = C[k][j] = float(p2[q])
            c = [float(p2[len(iu) + k]) for k in range(K)]
            cyy = float(p2[len(iu) + K])
            res = solve(K, sw, my, ms, C, c, cyy, standardize, float(ridge))
            if res is not None:
                GAMMA[t] = res[0]
                R2[t] = res[1]
    return dict(GAMMA=GAMMA, R2=R2, NOBS=NOBS, MY=MY)


def default_lags(T):
    """Engine.newey_west's default: floor(4 (T / 100)^(2/9))."""
    return int(math.floor(4.0 * (T / 100.0) ** (2.0 / 9.0)))


def newey_west(G, lags):
    """R6 per column of G [T][C] (or [T]) -> dict(MEAN, SE, T, NT int32), each [C] (or scalars'
    arrays of shape ()).  Non-NaN entries in time order x_1..x_n; mean = (sum x) / n;
    u = x - mean; a_l = (sum_{i > l} u_i * u_{i-l}) / n; var = a_0 + sum_l (2 (1 - l / (L + 1)))
    * a_l; SE = sqrt(var / n), T = mean / SE iff n >= L + 2 and var > 0."""
    G = np.asarray(G, dtype=np.float64)
    one = G.ndim == 1
    G2 = G[:, None] if one else G
    T, C = G2.shape
    L = int(lags)
    assert L >= 0
    MEAN = np.full(C, np.nan)
    SE = np.full(C, np.nan)
    TS = np.full(C, np.nan)
    NT = np.zeros(C, dtype=np.int32)
    for col in range(C):
        x = [float(v) for v in G2[:, col] if not math.isnan(v)]
        n = len(x)
        NT[col] = n
        if n == 0:
            continue
        sm = 0.0
        for v in x:
            sm = sm + v
        mean = sm / float(n)
        MEAN[col] = mean
        if n < L + 2:
            continue
        u = [v - mean for v in x]
        var = 0.0
        for l in range(L + 1):
            a = 0.0
            for i in range(l, n):
                a = a + u[i] * u[i - l]
            a = a / float(n)
            if l == 0:
                var = a
            else:
                var = var + (2.0 * (1.0 - float(l) / (float(L) + 1.0))) * a
        if var > 0.0:
            SE[col] = math.sqrt(var / float(n))
            TS[col] = mean / SE[col]
    out = dict(MEAN=MEAN, SE=SE, T=TS, NT=NT)
    return {k: v[0] for k, v in out.items()} if one else out


_INPUTS = {}
REAL_CASE = (24, 11, 1, 18)   # market_ref's (Wb, J, skip, min_obs) behind BETA and IVOL


def real_inputs(N):
    """The tests' real signals on market_ref.panel(N, "gappy"), 60 months: dict(PM, Y, S, X) with
    S = [mom_12,1, BETA, IVOL] at REAL_CASE on the fsum market and Y = the momentum ranking's
    next return; X is the B1 month return.  Made once and left unchanged."""
    if N not in _INPUTS:
        import market_ref as MR
        from oracle import csmom_oracle as O
        PM = MR.panel(N, "gappy")["PM"]
        mf = MR.market_factor(PM)
        mm = MR.market_model(PM, mf["MKT"], *REAL_CASE)
        scan = O.momentum_scan(PM, 12, 1)
        _INPUTS[N] = dict(PM=PM, Y=scan[2], S=[scan[1], mm["BETA"], mm["IVOL"]], X=mf["X"])
    return _INPUTS[N]


def wide_inputs():
    """The 20,001 x 14 panel of ten slices: S = [mom_3,1, the B1 return, a seeded normal array
    with 5 % NaN holes], Y = the momentum ranking's next return."""
    if "wide" not in _INPUTS:
        import market_ref as MR
        from oracle import csmom_oracle as O
        from oracle.synth_np import make_panel
        N = 20001
        pan = make_panel(N, 320, seed=300 + N, cents=True, with_volume=False, **MR.GAPPY)
        PM = O.month_end(pan["P"], pan["month_start"])[0][:14].copy()
        scan = O.momentum_scan(PM, 3, 1)
        _INPUTS["wide"] = dict(PM=PM, Y=scan[2],
                               S=[scan[1], MR.month_returns(PM), normal_panel(14, N, 1, 77)[0]])
    return _INPUTS["wide"]


def normal_panel(T_m, N, K, seed, holes=0.05):
    """K seeded standard-normal arrays [T_m][N], each with `holes` of its cells NaN."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        s = rng.normal(size=(T_m, N))
        s[rng.random((T_m, N)) < holes] = np.nan
        out.append(s)
    return out


def fama_macbeth(Y, S, W=None, standardize=True, ridge=0.0, min_obs=None, lags=None):
    """The two steps chained: xs_regress, then newey_west over GAMMA's columns and R2's mean."""
    r = xs_regress(Y, S, W, standardize, ridge, min_obs)
    L = default_lags(r["GAMMA"].shape[0]) if lags is None else int(lags)
    nw = newey_west(r["GAMMA"], L)
    r2 = newey_west(r["R2"], L)
    return dict(r, nw=nw, R2_MEAN=r2["MEAN"], lags=L)

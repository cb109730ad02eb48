"""Loop-level NumPy restatement of rules V1..V4: daily returns with a gap
bound, the equal-weight daily market, each (month, asset)'s raw moment sums and the window model
on them -- daily beta, idiosyncratic and total volatility, skewness, MAX.  A helper for the tests,
not a test file and not part of the product.  Loops run over days and months; every step is
elementwise over the assets, so each asset's sums are sequential in the stated order and no
operation is fused.  The market's sum over the assets is rule R1's (xsreg_ref.r1_sum).

  V1  d' = the latest priced row before d (priced = not NaN; the ABSENT payload is a NaN):
      r[d] = P[d] / P[d'] - 1  iff P[d] is priced, d' exists and d - d' <= max_gap (panel rows);
      else NaN.  Never month-bounded.
  V2  NMD[d] = the assets with r[d] not NaN;  MKTD[d] = r1_sum(r[d], NaN as 0.0) / NMD[d]
      iff NMD[d] >= min_assets, else NaN
  V3  per (month t, asset), days d of [month_start[t], month_start[t+1]) with r[d] and FD[d] not
      NaN, in day order from 0:  NO += 1, SR += r, SF += f, SRR += r*r, SFF += f*f, SRF += r*f,
      SR3 += (r*r)*r, RMAX = the largest r (NaN if none)
  V4  over months j = t-Wm+1 .. t (t-Wm+1 >= 0), each sum added oldest first from 0.0, n = sum NO,
      nf = float(n):  mr = SR/nf, mf = SF/nf, cff = SFF - SF*mf, crf = SRF - SR*mf,
      crr = SRR - SR*mr;
      DBETA = crf/cff  iff n >= min_obs and cff > 0
      DIVOL = sqrt(max(q, 0)/(nf - 2)), q = crr - DBETA*crf  iff DBETA defined and n >= 3
      DTVOL = sqrt(crr/(nf - 1))  iff n >= min_obs, n >= 2, crr >= 0
      DSKEW = m3/(v*sqrt(v)), v = crr/nf, m3 = (SR3 - (3*mr)*SRR + ((2*SR)*mr)*mr)/nf
              iff n >= min_obs, n >= 3, v > 0
      DMAX  = the largest non-NaN RMAX[j]  iff n >= min_obs;   NOBS = n (0 before a whole window)
"""
import numpy as np

from xsreg_ref import r1_sum


def daily_ret(P, max_gap=10):
    """V1 -> r [T_d][N]."""
    T_d, N = P.shape
    r = np.full((T_d, N), np.nan)
    last = np.full(N, np.nan)                  # price of the latest priced row so far
    at = np.full(N, -1, dtype=np.int64)        # its row, -1: none
    with np.errstate(invalid="ignore", divide="ignore"):
        for d in range(T_d):
            x = P[d]
            ok = ~np.isnan(x)
            have = ok & (at >= 0) & (d - at <= max_gap)
            q = x / last - 1.0
            r[d] = np.where(have, q, np.nan)
            last = np.where(ok, x, last)
            at = np.where(ok, d, at)
    return r


def daily_market(P, max_gap=10, min_assets=1):
    """V1, V2 -> dict(R [T_d][N], MKTD [T_d], NMD [T_d] int32)."""
    r = daily_ret(P, max_gap)
    obs = ~np.isnan(r)
    nmd = obs.sum(axis=1).astype(np.int32)
    s = r1_sum(np.where(obs, r, 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        mktd = np.where(nmd >= min_assets, s / nmd.astype(np.float64), np.nan)
    return dict(R=r, MKTD=mktd, NMD=nmd)


SUMS = ("NO", "SR", "SF", "SRR", "SFF", "SRF", "SR3", "RMAX")


def daily_sums(R, FD, month_start):
    """V3 on V1's returns R -> dict of SUMS, each [T_m][N] (NO int32)."""
    T_d, N = R.shape
    T_m = len(month_start) - 1
    out = {k: np.zeros((T_m, N)) for k in SUMS[1:7]}
    out["NO"] = np.zeros((T_m, N), dtype=np.int32)
    out["RMAX"] = np.full((T_m, N), np.nan)
    for t in range(T_m):
        no = np.zeros(N, dtype=np.int32)
        sr, sf, srr, sff, srf, sr3 = (np.zeros(N) for _ in range(6))
        rmax = np.full(N, np.nan)
        for d in range(int(month_start[t]), int(month_start[t + 1])):
            r = R[d]
            f = np.full(N, FD[d])
            obs = ~np.isnan(r) & ~np.isnan(f)
            rr = r * r
            ff = f * f
            rf = r * f
            r3 = rr * r
            no = no + obs
            sr = np.where(obs, sr + r, sr)
            sf = np.where(obs, sf + f, sf)
            srr = np.where(obs, srr + rr, srr)
            sff = np.where(obs, sff + ff, sff)
            srf = np.where(obs, srf + rf, srf)
            sr3 = np.where(obs, sr3 + r3, sr3)
            with np.errstate(invalid="ignore"):
                rmax = np.where(obs & (np.isnan(rmax) | (r > rmax)), r, rmax)
        out["NO"][t], out["SR"][t], out["SF"][t], out["SRR"][t] = no, sr, sf, srr
        out["SFF"][t], out["SRF"][t], out["SR3"][t], out["RMAX"][t] = sff, srf, sr3, rmax
    return out


MODEL = ("DBETA", "DIVOL", "DTVOL", "DSKEW", "DMAX", "NOBS")


def daily_model(sums, Wm=1, min_obs=None):
    """V4 -> dict of MODEL, each [T_m][N] (NOBS int32)."""
    T_m, N = sums["SR"].shape
    min_obs = 15 * Wm if min_obs is None else min_obs
    out = {k: np.full((T_m, N), np.nan) for k in MODEL[:5]}
    out["NOBS"] = np.zeros((T_m, N), dtype=np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(Wm - 1, T_m):
            n = np.zeros(N, dtype=np.int64)
            SR, SF, SRR, SFF, SRF, SR3 = (np.zeros(N) for _ in range(6))
            mx = np.full(N, np.nan)
            for j in range(t - Wm + 1, t + 1):
                n = n + sums["NO"][j]
                SR = SR + sums["SR"][j]
                SF = SF + sums["SF"][j]
                SRR = SRR + sums["SRR"][j]
                SFF = SFF + sums["SFF"][j]
                SRF = SRF + sums["SRF"][j]
                SR3 = SR3 + sums["SR3"][j]
                x = sums["RMAX"][j]
                mx = np.where(~np.isnan(x) & (np.isnan(mx) | (x > mx)), x, mx)
            nf = n.astype(np.float64)
            mr = SR / nf
            mf = SF / nf
            cff = SFF - SF * mf
            crf = SRF - SR * mf
            crr = SRR - SR * mr
            enough = n >= min_obs
            bdef = enough & (cff > 0.0)
            beta = np.where(bdef, crf / cff, np.nan)
            q = crr - beta * crf
            qp = np.where(q < 0.0, 0.0, q)
            ivol = np.where(bdef & (n >= 3), np.sqrt(qp / (nf - 2.0)), np.nan)
            tvol = np.where(enough & (n >= 2) & (crr >= 0.0), np.sqrt(crr / (nf - 1.0)), np.nan)
            v = crr / nf
            t1 = (3.0 * mr) * SRR
            t2 = ((2.0 * SR) * mr) * mr
            m3 = ((SR3 - t1) + t2) / nf
            skew = np.where(enough & (n >= 3) & (v > 0.0), m3 / (v * np.sqrt(v)), np.nan)
            out["DBETA"][t], out["DIVOL"][t], out["DTVOL"][t] = beta, ivol, tvol
            out["DSKEW"][t] = skew
            out["DMAX"][t] = np.where(enough, mx, np.nan)
            out["NOBS"][t] = n
    return out


def gap_column(T_d, max_gap, straddle, absent):
    """A hand-built price column with gaps of exactly max_gap - 1, max_gap and max_gap + 1 rows
    between priced rows (d - d'), each once with NaN rows and once with ABSENT rows in between.
    The gaps end 14 rows apart at rows 0 or 1 past a multiple of 7, so with 7-day chunks every
    one crosses a chunk start; one more gap of max_gap rows ends at row straddle + 1, its rows
    without a price on both sides of `straddle` (a month start).  Returns (column, cases), cases a
    list of (d, d', booked)."""
    col = 20.0 + 0.25 * np.arange(T_d) + (np.arange(T_d) % 5) * 0.07
    cases = []
    i = 0
    for g in (max_gap - 1, max_gap, max_gap + 1):
        for hole in (np.nan, absent):
            d = 14 * (i + 1) + (i % 2)
            i += 1
            if g < 1:
                continue
            col[d - g + 1:d] = hole
            cases.append((d, d - g, g <= max_gap))
    d = straddle + 1
    assert d - max_gap > 14 * i + 3 and max_gap >= 2 and d < T_d
    col[d - max_gap + 1:d] = np.nan
    cases.append((d, d - max_gap, True))
    return col, cases


def daily(P, month_start, max_gap=10, min_assets=1, FD=None):
    """V1..V3 end to end: daily_market's dict plus SUMS on FD (None: MKTD)."""
    out = daily_market(P, max_gap, min_assets)
    out.update(daily_sums(out["R"], out["MKTD"] if FD is None else FD, month_start))
    return out

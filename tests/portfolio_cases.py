"""Synthetic portfolio-accounting panels that cross the kernel-selection thresholds of
csrc/portfolio.hip -- the case builder shared by tests/test_portfolio_cases_cpu.py (which proves
on the CPU oracle that every case contains what it claims) and tests/test_gpu_portfolio_horizons.py
(which runs them on the engine against oracle.portfolio_oracle.portfolio).

A plain module, not a conftest: it imports the oracle and never edits it.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np

from oracle import portfolio_oracle as PO

# ---------------------------------------------------------------- thresholds of portfolio.hip
# (tests/test_portfolio_cases_cpu.py parses the source and fails when one of them moves)
PF_CHUNK_MIN = 256   # assets per chunk: N = 260 rows have two turnover chunks
TP_U = 16            # k_turn_prep loads the formation totals in trips of TP_U ages
BM_MAXK = 31         # `kq <= 31`: general equal-weight rows take k_turnover<.., BM=true> up to it
OV_TRIP = 8          # k_overlap_rows walks the ages in trips of OV_TRIP
TO_GEN_TB = 8        # general rows: tables for ages 0..TO_GEN_TB-1, then a walk over the rest
AC_MAXKD = 384       # k_cohort_lds while K * n_bins <= AC_MAXKD, else k_cohort
SEG_MAXKD = 512      # segment path while K * (n_bins + 1) <= SEG_MAXKD
SEG_MAXN = 7168      # widest row of the segment path
TO_MAXQ = 4          # holding periods per accounting batch
TO_MAXK = 240        # largest holding period accepted
LS_PB = 64           # batches of >= LS_PB panels take the two-launch long-short

AUM = 5e6
REL = 1e-10


def k_lists():
    """{n_bins: sorted K list} on both sides of every K threshold, derived from the constants."""
    nb10 = {TO_GEN_TB, TO_GEN_TB + 1,                # tables only / tables + walk
            OV_TRIP + 5,                             # Kmax > OV_TRIP, not a multiple of it
            TP_U - 1, TP_U, TP_U + 1,                # one / two k_turn_prep trips
            2 * TP_U - 1, 2 * TP_U, 2 * TP_U + 1,    # two / three trips
            BM_MAXK, BM_MAXK + 1,                    # bitmask general rows / plain
            AC_MAXKD // 10, AC_MAXKD // 10 + 1,
            SEG_MAXKD // 11, SEG_MAXKD // 11 + 1,
            4 * TP_U,                                # a multiple of both trip lengths, past every limit
            TO_MAXK}
    nb30 = {AC_MAXKD // 30, AC_MAXKD // 30 + 1, SEG_MAXKD // 31, SEG_MAXKD // 31 + 1}
    nb2 = {SEG_MAXKD // 3, SEG_MAXKD // 3 + 1, AC_MAXKD // 2, AC_MAXKD // 2 + 1}
    return {10: sorted(nb10), 30: sorted(nb30), 2: sorted(nb2)}


def k_all_costs():      # every cost model (equal / value weights x impact or not)
    return (BM_MAXK, BM_MAXK + 1, TO_MAXK)


def k_odd_widths():     # repeated at N = 259 and 258 (scalar label loads, no bitmask kernel)
    return (TP_U + 1, 2 * TP_U + 1, SEG_MAXKD // 11 + 1)


def k_forced_modes():   # repeated under each forced cohort kernel
    return (TP_U + 1, SEG_MAXKD // 11 + 1)


# ---------------------------------------------------------------- cases
ALL_PLANTS = ("empty_top", "blank_month", "nan_month", "dead_weights", "no_top_ever")
FULL = ("steady", "nonfull", "pr_nan", "pr_finite", "turn_finite", "turn0")


@dataclass(frozen=True)
class Case:
    """One synthetic panel.  K is the holding period the claims are checked at (the longest of
    a K set).  label_seed: labels from another stream than NR / W / ADV / SIG (look-backs that
    share one next-return panel)."""
    T_m: int
    B: int
    N: int
    n_bins: int
    seed: int
    vw: bool
    plant: tuple
    K: int
    claims: tuple
    label_seed: int | None = None


def plant_months(T_m):
    """Where the planted months go.  Month 0 stays clean (TURN[0] == 1), the head holds two
    top-less months and the dead-weights month, the tail the blank month and the third top-less
    month; the NaN-return month (which empties no cohort) is mid-panel.  Rows t in [K + 4,
    T_m - 3] keep every window full."""
    assert T_m >= 8, "planted months need T_m >= 8"
    return dict(empty_top=(1, 3, T_m - 1), dead_weights=2, blank_month=T_m - 2, nan_month=T_m // 2)


def make_case(T_m, B, N, n_bins, seed, vw, plant=(), label_seed=None):
    """Host arrays L int8, NR, W (None for equal weights), ADV, SIG, each [T_m][B][N]."""
    assert set(plant) <= set(ALL_PLANTS), plant
    assert "dead_weights" not in plant or vw
    assert "no_top_ever" not in plant or B >= 2
    rl = np.random.default_rng([seed if label_seed is None else label_seed, 1])
    rd = np.random.default_rng([seed, 2])
    shape = (T_m, B, N)
    L = rl.integers(-1, n_bins, shape).astype(np.int8)
    NR = rd.normal(0.01, 0.08, shape)
    NR[rd.random(shape) < 0.05] = np.nan
    ADV = rd.uniform(1e5, 1e8, shape)
    ADV[rd.random(shape) < 0.005] = 0.0
    SIG = rd.uniform(0.005, 0.05, shape)
    SIG[rd.random(shape) < 0.02] = np.nan
    W = rd.uniform(1e6, 1e9, shape)
    u = rd.random(shape)
    W[u < 0.01] = np.nan
    W[(u >= 0.01) & (u < 0.02)] = -1.0
    top = n_bins - 1
    low = top - 1 if n_bins > 2 else -1    # where a removed top label goes
    if plant:
        pm = plant_months(T_m) if set(plant) - {"no_top_ever"} else {}
    if "empty_top" in plant:
        for t in pm["empty_top"]:
            L[t, 0][L[t, 0] == top] = low
    if "blank_month" in plant:
        L[pm["blank_month"], 0] = -1
    if "nan_month" in plant:
        NR[pm["nan_month"], 0] = np.nan
    if "dead_weights" in plant:
        W[pm["dead_weights"], 0, 0::2] = np.nan
        W[pm["dead_weights"], 0, 1::2] = -1.0
    if "no_top_ever" in plant:
        L[:, 1][L[:, 1] == top] = low
    return dict(L=L, NR=NR, W=W if vw else None, ADV=ADV, SIG=SIG)


@lru_cache(maxsize=None)
def arrays(case: Case):
    """The case's arrays, built once and shared (read-only) by every test that uses it."""
    a = make_case(case.T_m, case.B, case.N, case.n_bins, case.seed, case.vw, case.plant,
                  case.label_seed)
    for v in a.values():
        if v is not None:
            v.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def oracle_ref(case: Case, K: int, impact: bool):
    """PO.portfolio of the case at holding period K, computed once per process."""
    a = arrays(case)
    kw = dict(aum=AUM, ADV=a["ADV"], SIG=a["SIG"]) if impact else {}
    r = PO.portfolio(a["L"], a["NR"], case.n_bins, K=K, W=a["W"], **kw)
    return {f: r[f] for f in ("PR", "LS", "TURN", "COST", "NET")}


def _claims(case_plant, T_m, K, extra=()):
    c = list(FULL if T_m > K else ("no_row_ge_K",) + FULL[2:])
    if "no_top_ever" in case_plant:
        c.append("ls_fallback")
    return tuple(c) + tuple(extra)


def _mk(T_m, B, N, n_bins, seed, vw, plant, K, claims=None, label_seed=None):
    plant = tuple(p for p in plant if vw or p != "dead_weights")
    return Case(T_m, B, N, n_bins, seed, vw, plant, K,
                _claims(plant, T_m, K) if claims is None else claims, label_seed)


PLANT_A = ("empty_top", "blank_month", "nan_month", "no_top_ever")


def group_a():
    """[(id, case, impact, cohort mode or None)]: every K of k_lists() at T_m = K + 9, B = 2,
    N = 260, equal weights without impact and value weights with impact; the extra cost
    models, row widths and forced cohort kernels of the issue."""
    out = []
    for nb, Ks in k_lists().items():
        for K in Ks:
            ew = _mk(K + 9, 2, 260, nb, 1000 + K, False, PLANT_A, K)
            vw = replace(ew, vw=True)
            out.append((f"nb{nb}-K{K}-ew", ew, False, None))
            out.append((f"nb{nb}-K{K}-vw-imp", vw, True, None))
            if nb == 10 and K in k_all_costs():
                out.append((f"nb{nb}-K{K}-ew-imp", ew, True, None))
                out.append((f"nb{nb}-K{K}-vw", vw, False, None))
            if nb == 10 and K in k_odd_widths():
                for N in (259, 258):
                    out.append((f"nb{nb}-K{K}-ew-N{N}", replace(ew, N=N), False, None))
            if nb == 10 and K in k_forced_modes():
                for mode in ("seg", "lds"):
                    out.append((f"nb{nb}-K{K}-ew-{mode}", ew, False, mode))
                    out.append((f"nb{nb}-K{K}-vw-imp-{mode}", vw, True, mode))
    return out


KS_NINE = (12, 1, 7, 3, 24, 5, 36, 2, 18)   # unsorted; batches (12,1,7,3) (24,5,36,2) (18)
KS_FIVE = (33, 6, 6, 40, 2)                 # one repeated; the second batch is (2,)
PLANT_B = ("empty_top", "blank_month", "nan_month")


def group_b():
    """[(id, case, Ks, opts)]: K sets longer than TO_MAXQ, T_m = 50, n_bins = 10."""
    assert len(KS_NINE) > 2 * TO_MAXQ and len(KS_FIVE) == TO_MAXQ + 1
    out = []
    for tag, Ks in (("nine", KS_NINE), ("five", KS_FIVE)):
        K = max(Ks)
        c1 = _mk(50, 1, 260, 10, 2001, True, PLANT_B + ("dead_weights",), K)
        c3 = _mk(50, 3, 260, 10, 2003, False, PLANT_B + ("no_top_ever",), K)
        c3p = _mk(50, 3, 260, 10, 2004, False, PLANT_B, K)
        c70 = _mk(50, LS_PB + 6, 64, 10, 2070, False, PLANT_B + ("no_top_ever",), K)
        out += [(f"{tag}-B1-vw-imp", c1, Ks, dict(impact=True)),
                (f"{tag}-B3-ew", c3, Ks, dict()),
                (f"{tag}-B70-ew-N64", c70, Ks, dict()),
                (f"{tag}-B3-nocosts", c3, Ks, dict(with_costs=False)),
                (f"{tag}-B3-legs-needfull", c3, Ks, dict(legs_only=True, need_full=True)),
                (f"{tag}-B3-legs", c3p, Ks, dict(legs_only=True, need_full=False)),
                (f"{tag}-B70-legs-needfull", c70, Ks, dict(legs_only=True, need_full=True))]
    return out


def group_b_grouped():
    """G = 2 groups of Bg = 2 panels, value weights shared by the groups, the nine-entry set."""
    return _mk(50, 4, 260, 10, 2104, True, PLANT_B + ("dead_weights", "no_top_ever"), max(KS_NINE))


def group_c():
    """[(id, case, impact)]: histories around and below the holding period."""
    out = []
    for K in (6, 40):
        for T_m in (1, 2, K - 1, K, K + 1):
            for N in (260, 259):
                ew = _mk(T_m, 2, N, 10, 3000 + K, False, ("no_top_ever",), K)
                out.append((f"K{K}-T{T_m}-N{N}-ew", ew, False))
                out.append((f"K{K}-T{T_m}-N{N}-vw-imp", replace(ew, vw=True), True))
    return out


def group_d():
    """[(id, case)]: rows narrower than a wave; most deciles are empty."""
    out = []
    for N in (1, 3, 4, 5, 63, 64, 65):
        for nb in (2, 10):
            for vw in (False, True):
                # fewer assets than deciles: some decile is empty in every month
                claims = ("pr_finite", "turn_finite") + (("pr_nan",) if N < nb else ())
                c = _mk(12, 3, N, nb, 4000 + N, vw, (), 3, claims=claims)
                out.append((f"N{N}-nb{nb}-{'vw' if vw else 'ew'}", c))
    return out


def group_e():
    """[(id, case)]: batched value weights with a dead-weights month and impact costs."""
    out = []
    for B in (3, 16):
        for K in (6, 2 * TP_U + 1):
            c = _mk(K + 9, B, 260, 10, 5000 + B, True, PLANT_A + ("dead_weights",), K)
            out.append((f"B{B}-K{K}", c))
    return out


def js_cases(T_m, B, N, K, nJ, seed):
    """nJ label panels (labels from nJ seeds) over ONE next-return panel."""
    return [_mk(T_m, B, N, 10, seed, False, PLANT_B, K, label_seed=seed + 1 + q) for q in range(nJ)]


F1_KS = ((3, SEG_MAXKD // 44), (3, SEG_MAXKD // 44 + 1))   # 4 * K * 11 <= / > SEG_MAXKD: (3, 11), (3, 12)
F2_KS = (6, 60)
F3_KS = ((3, SEG_MAXKD // 16), (3, SEG_MAXKD // 16 + 1))   # 4 * K * 4 <= / > SEG_MAXKD: (3, 32), (3, 33)


def group_f1(Ks):
    return js_cases(140, 8, 64, max(Ks), 4, 6000)


def group_f2():
    return js_cases(69, 60, 64, max(F2_KS), 2, 6100)


def group_f3(Ks):
    return js_cases(69, 60, 64, max(Ks), 4, 6100)


def all_cases():
    """Every (case) the GPU file builds, once."""
    cs = [g[1] for g in group_a()] + [g[1] for g in group_b()] + [group_b_grouped()]
    cs += [g[1] for g in group_c()] + [g[1] for g in group_d()] + [g[1] for g in group_e()]
    for Ks in F1_KS:
        cs += group_f1(Ks)
    cs += group_f2()
    for Ks in F3_KS:
        cs += group_f3(Ks)
    seen, out = set(), []
    for c in cs:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


# ---------------------------------------------------------------- what a case contains
def leg_nonempty(case: Case):
    """ne[t][b][leg]: the cohort formed in month t has a member in the leg (top, bottom)."""
    a = arrays(case)
    return np.stack([PO.member_weights(a["L"], d, a["W"]).sum(axis=2) > 0
                     for d in (case.n_bins - 1, 0)], axis=2)


def row_classes(case: Case, K: int):
    """(steady, nonfull) bool [T_m][B]: rows t >= K whose windows of months t and t - 1 (the
    formation months t - K .. t) are all non-empty in both legs, and rows t >= K where one is
    not."""
    ne = leg_nonempty(case).all(axis=2)
    T_m, B = ne.shape
    steady = np.zeros((T_m, B), dtype=bool)
    nonfull = np.zeros((T_m, B), dtype=bool)
    for t in range(K, T_m):
        full = ne[t - K:t + 1].all(axis=0)
        steady[t], nonfull[t] = full, ~full
    return steady, nonfull

"""Momentum x trading-volume double sort (Lee & Swaminathan 2000, section II; SURVEY 8(f)
rank 3).  The reference computes share turnover (src/features.py:60-107) but never uses it;
this finishes the thought its LeSw00.pdf describes: stocks are sorted independently each
month into momentum deciles (the reference's qcut rule, run_demo.py:18-29) and turnover
terciles (the same rule with 3 bins on the rolling turnover, over the rows with a valid
signal), and the 30 cell portfolios are held K months (rules E1..E5 with 30 groups).

Everything runs on the device: csm_turnover_features, csm_deciles (twice),
csm_double_sort_labels, csm_portfolio (n_bins = 30).  Parity: the turnover features are
bit-exact with the reference (tests/golden/turnover.npz); the sort and cell returns are
pinned only by the oracle restatement (rule T2, oracle/features_oracle.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class DoubleSortResult:
    Lm: torch.Tensor          # [T_m][N] momentum decile
    Lv: torch.Tensor          # [T_m][N] turnover tercile
    Lc: torch.Tensor          # [T_m][N] cell = n_vol * Lm + Lv
    PR: torch.Tensor          # [T_m][n_mom][n_vol] cell returns (K-overlapped)
    LS: torch.Tensor          # [T_m][n_vol] top minus bottom momentum decile per tercile
    TAVG: torch.Tensor        # [T_m][N] rolling turnover used for the terciles


def momentum_volume_double_sort(eng, PM, VOL, M, NR, so, mcap, n_mom=10, n_vol=3, K=1,
                                lookback=3, W=None) -> DoubleSortResult:
    T_m, N = M.shape
    _, _, _, TAVG = eng.turnover_features(PM, VOL, so, mcap, lookback)
    Lm, _, _, _ = eng.deciles(M, None, n_mom)
    Lv, _, _, _ = eng.deciles(eng.mask_by(M, TAVG), None, n_vol)
    Lc = eng.combine_labels(Lm, Lv, n_vol)
    out = eng.portfolio(Lc, NR, n_mom * n_vol, K=K, W=W, with_costs=False)
    PR = out.PR[:, 0, :].reshape(T_m, n_mom, n_vol)
    LS = PR[:, n_mom - 1, :] - PR[:, 0, :]
    return DoubleSortResult(Lm=Lm, Lv=Lv, Lc=Lc, PR=PR, LS=LS, TAVG=TAVG)


@dataclass
class DependentSortResult:
    Lm: torch.Tensor          # [T_m][N] first sort's label (n1 bins of S1)
    Lv: torch.Tensor          # [T_m][N] second sort's label: n2 bins of S2 inside each first bin
    Lc: torch.Tensor          # [T_m][N] cell = n2 * Lm + Lv
    PR: torch.Tensor          # [T_m][n1][n2] cell returns (K-overlapped)
    LS: torch.Tensor          # [T_m][n1] top minus bottom second-sort bin per first bin


PORTFOLIO_BINS = (2, 3, 4, 5, 10, 20, 30)   # the group counts csm_portfolio accounts in one call


def cell_returns(eng, L1, L2, NR, n1, n2, K=1, W=None, joint=None, Lc=None):
    """[T_m][n1][n2] returns of the cells (first label, second label), held K months.  joint:
    the n1 * n2 cells as one csm_portfolio call on the combined labels (default: when n1 * n2
    is one of PORTFOLIO_BINS); otherwise the n1 first bins one call each, every one an n2-bin
    portfolio of the second labels inside it.  A cell's return depends on its own members
    alone, so both give the same cells.  Lc: combine_labels(L1, L2, n2) when the caller has it."""
    T_m, _ = L1.shape
    if joint is None:
        joint = n1 * n2 in PORTFOLIO_BINS
    if joint:
        Lc = eng.combine_labels(L1, L2, n2) if Lc is None else Lc
        out = eng.portfolio(Lc, NR, n1 * n2, K=K, W=W, with_costs=False)
        return out.PR[:, 0, :].reshape(T_m, n1, n2)
    none = torch.full_like(L2, -1)
    return torch.stack([eng.portfolio(torch.where(L1 == i, L2, none), NR, n2, K=K, W=W,
                                      with_costs=False).PR[:, 0, :] for i in range(n1)], dim=1)


def dependent_double_sort(eng, S1, S2, NR, n1=3, n2=10, K=1, W=None) -> DependentSortResult:
    """The conditional double sort: n1 bins of S1 per date, then n2 bins of S2 inside each of
    them (csm_group_deciles with the first labels as the groups, rules N1, N2), and the
    n1 * n2 cell portfolios held K months (cell_returns: any n1 with n2 one of
    PORTFOLIO_BINS)."""
    T_m, N = S1.shape
    L1, _, _, _ = eng.deciles(S1, None, n1)
    L2, _, _ = eng.deciles_within(S2, None, L1.to(torch.int16), n1, n2)
    Lc = eng.combine_labels(L1, L2, n2)
    PR = cell_returns(eng, L1, L2, NR, n1, n2, K, W, Lc=Lc)
    LS = PR[:, :, n2 - 1] - PR[:, :, 0]
    return DependentSortResult(Lm=L1, Lv=L2, Lc=Lc, PR=PR, LS=LS)


__all__ = ["DoubleSortResult", "DependentSortResult", "PORTFOLIO_BINS", "cell_returns",
           "dependent_double_sort",
           "momentum_volume_double_sort"]

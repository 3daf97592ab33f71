"""Fisher feature selection for ``ClusterCRF.fit(select=...)``: the counterpart of ``gecco.crf.select``
(``fisher_significance``, ``significance_correction``) and of the selection rule of ``gecco/crf/__init__.py:318-346``.

The contingency tables are counted on the host with numpy, the two-sided Fisher exact p-values come from the device
(``gecco_crf_fisher_exact``, ``csrc/crf_fisher.hip``), and the multiple-test corrections are statsmodels' (0.12)
``multipletests(..., is_sorted=True)`` restated in numpy with the same operations in the same order.
"""
import warnings
from typing import Any, Dict, FrozenSet, Iterable, List, Mapping, Optional, Tuple

import numpy as np

from . import _native

# statsmodels' names of the ten methods the reference accepts, with their aliases (matched after ``method.lower()``)
CORRECTION_ALIASES = {
    "bonferroni": ("b", "bonf", "bonferroni"),
    "sidak": ("s", "sidak"),
    "holm": ("h", "holm"),
    "holm-sidak": ("hs", "holm-sidak"),
    "simes-hochberg": ("sh", "simes-hochberg"),
    "hommel": ("ho", "hommel"),
    "fdr_bh": ("fdr_bh", "fdr_i", "fdr_p", "fdri", "fdrp"),
    "fdr_by": ("fdr_by", "fdr_n", "fdr_c", "fdrn", "fdrcorr"),
    "fdr_tsbh": ("fdr_tsbh", "fdr_2sbh"),
    "fdr_tsbky": ("fdr_tsbky", "fdr_2sbky", "fdr_twostage"),
}
_CANONICAL = {alias: name for name, aliases in CORRECTION_ALIASES.items() for alias in aliases}
_ALPHA = 0.05  # multipletests' default, which the reference does not override (the two-stage methods depend on it)

SELECT_WARNING = "Selected features still include domains with a p-value of 1, consider reducing the selected fraction."


def fisher_exact_pvalues(tables: Any, device: int = 0) -> np.ndarray:
    """Two-sided Fisher exact p-values of ``tables`` (``(n, 2, 2)`` or ``(n, 4)`` non-negative integers, ``[[a, b], [c, d]]``)
    on the device: ``scipy.stats.fisher_exact(table, alternative="two-sided").pvalue`` of every table, in fp64."""
    return _native.fisher_exact(tables, device=device)


def contingency_tables(proteins: Iterable[Any]) -> Tuple[List[str], np.ndarray]:
    """The tables ``fisher_significance`` tests: for every domain name seen, ``[[a, Nc - a], [b, Nn - b]]`` with ``a`` / ``b``
    the numbers of in-cluster / not-in-cluster proteins carrying it and ``Nc`` / ``Nn`` the numbers of proteins of each class.

    Counting follows the reference's sets keyed by protein id: a domain is in a cluster when its ``probability > 0.5``; a
    protein counts once per class however many domains put it there (repeated domains and genes sharing a protein id count
    once), in both classes if its domains have both, and nowhere without domains.  Names are returned sorted."""
    pid_of: Dict[str, int] = {}
    fid_of: Dict[str, int] = {}
    pids: List[int] = []
    fids: List[int] = []
    probs: List[float] = []
    for protein in proteins:
        domains = protein.domains
        if not domains:
            continue
        pid = pid_of.setdefault(protein.id, len(pid_of))
        for domain in domains:
            if domain.probability is None:
                raise ValueError("Domain is missing a gene cluster probability")
            pids.append(pid)
            fids.append(fid_of.setdefault(domain.name, len(fid_of)))
            probs.append(domain.probability)
    names = sorted(fid_of)
    if not names:
        return names, np.zeros((0, 2, 2), dtype=np.int64)
    rank = np.empty(len(fid_of), dtype=np.int64)  # interned id -> position among the sorted names
    rank[[fid_of[name] for name in names]] = np.arange(len(names))
    pid = np.asarray(pids, dtype=np.int64)
    fid = rank[np.asarray(fids, dtype=np.int64)]
    cls = (np.asarray(probs, dtype=np.float64) > 0.5).astype(np.int64)
    n_prot = len(pid_of)
    # proteins of each class: distinct (protein, class)
    prot_cls = np.unique(pid * 2 + cls)
    n_class = np.bincount(prot_cls & 1, minlength=2)
    # proteins of each class with each feature: distinct (feature, protein, class)
    triple = np.unique((fid * n_prot + pid) * 2 + cls)
    feat, tcls = triple // (2 * n_prot), triple & 1
    with_f = np.bincount(feat * 2 + tcls, minlength=2 * len(names)).reshape(len(names), 2)
    tables = np.empty((len(names), 2, 2), dtype=np.int64)
    tables[:, 0, 0] = with_f[:, 1]
    tables[:, 0, 1] = n_class[1] - with_f[:, 1]
    tables[:, 1, 0] = with_f[:, 0]
    tables[:, 1, 1] = n_class[0] - with_f[:, 0]
    return names, tables


def fisher_significance(proteins: Iterable[Any], correction_method: Optional[str] = "fdr_bh", *,
                        device: int = 0) -> Dict[str, float]:
    """The significance of every domain name of ``proteins`` (``gecco.crf.select.fisher_significance``): the two-sided
    Fisher exact p-value of its contingency table (``contingency_tables``), corrected with ``correction_method`` unless it
    is None.  Values are Python floats."""
    if correction_method is not None:
        _canonical(correction_method)  # (an unknown name fails before any work)
    names, tables = contingency_tables(proteins)
    pvalues = fisher_exact_pvalues(tables, device=device) if len(names) else np.zeros(0)
    significance = dict(zip(names, pvalues.tolist()))
    if correction_method is not None:
        significance = significance_correction(significance, correction_method)
    return significance


def _canonical(method: str) -> str:
    try:
        return _CANONICAL[method.lower()]
    except KeyError:
        raise ValueError("method not recognized") from None


def _fdrcorrection(p: np.ndarray, alpha: float, negcorr: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    ecdffactor = np.arange(1, len(p) + 1) / float(len(p))
    if negcorr:
        cm = np.sum(1. / np.arange(1, len(p) + 1))
        ecdffactor = ecdffactor / cm
    reject = p <= ecdffactor * alpha
    if reject.any():
        reject[:max(np.nonzero(reject)[0])] = True
    corrected = np.minimum.accumulate((p / ecdffactor)[::-1])[::-1]
    corrected[corrected > 1] = 1
    return reject, corrected


def _fdr_twostage(p: np.ndarray, alpha: float, bky: bool) -> np.ndarray:
    n = len(p)
    fact = (1. + alpha) if bky else 1.
    alpha_prime = alpha / fact if bky else alpha
    rej, corrected = _fdrcorrection(p, alpha_prime)
    r1 = rej.sum()
    if r1 == 0 or r1 == n:
        return corrected * fact
    n0 = 1.0 * n - r1
    alpha_star = alpha_prime * n / n0
    _, corrected = _fdrcorrection(p, alpha_star)
    corrected *= n0 * 1.0 / n
    if bky:
        corrected *= (1. + alpha)
    return corrected


def _corrected(p: np.ndarray, method: str) -> np.ndarray:
    """statsmodels 0.12 ``multipletests(p, method=method, is_sorted=True)[1]`` for ascending ``p``."""
    n = len(p)
    if method == "bonferroni":
        out = p * float(n)
    elif method == "sidak":
        out = 1 - np.power((1. - p), n)
    elif method == "holm-sidak":
        out = np.maximum.accumulate(1 - np.power((1. - p), np.arange(n, 0, -1)))
    elif method == "holm":
        out = np.maximum.accumulate(p * np.arange(n, 0, -1))
    elif method == "simes-hochberg":
        out = np.minimum.accumulate((np.arange(n, 0, -1) * p)[::-1])[::-1]
    elif method == "hommel":
        out = p.copy()
        for m in range(n, 1, -1):
            cim = np.min(m * p[-m:] / np.arange(1, m + 1.))
            out[-m:] = np.maximum(out[-m:], cim)
            out[:-m] = np.maximum(out[:-m], np.minimum(m * p[:-m], cim))
    elif method == "fdr_bh":
        out = _fdrcorrection(p, _ALPHA)[1]
    elif method == "fdr_by":
        out = _fdrcorrection(p, _ALPHA, negcorr=True)[1]
    elif method == "fdr_tsbh":
        out = _fdr_twostage(p, _ALPHA, bky=False)
    else:  # fdr_tsbky
        out = _fdr_twostage(p, _ALPHA, bky=True)
    out[out > 1] = 1
    return out


def significance_correction(significance: Mapping[str, float], method: str) -> Dict[str, float]:
    """Multiple-test correction of ``significance`` (``gecco.crf.select.significance_correction``): the p-values sorted
    ascending (ties by name) go through statsmodels' ``multipletests(..., method=method, is_sorted=True)``, restated here;
    ``method`` is one of the ten methods the reference accepts or a statsmodels alias of one (``ValueError`` otherwise)."""
    canonical = _canonical(method)
    features = sorted(significance, key=lambda name: (significance[name], name))
    if not features:
        return {}
    p = np.array([significance[name] for name in features], dtype=np.float64)
    return dict(zip(features, _corrected(p, canonical).tolist()))


def select_features(significance: Mapping[str, float], select: float) -> FrozenSet[str]:
    """The selection rule of ``ClusterCRF.fit(select=...)``: the ``int(select * len(significance))`` names with the smallest
    p-values (ties broken by name), warning when the cut still takes a p-value of 1."""
    if not (0 < select <= 1):
        raise ValueError(f"invalid value for select: {select}")
    k = int(select * len(significance))
    if k == 0:
        raise ValueError(f"select={select} selects no feature out of {len(significance)}")
    chosen = sorted(significance, key=lambda name: (significance[name], name))[:k]
    if significance[chosen[-1]] == 1.0:
        warnings.warn(SELECT_WARNING, UserWarning)
    return frozenset(chosen)

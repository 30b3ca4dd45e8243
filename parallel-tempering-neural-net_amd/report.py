"""Classification report of the drop-in (not in the reference, which publishes accuracy only): which class is taken for which, per-class
precision, recall and F1, one-vs-rest ROC-AUC -- of the pooled (posterior-mean) classifier, and of every sampled net, so that each
figure comes with its spread over the posterior.  The host-only helpers, the result tuple, and the mixin that holds the public
method.  The method checks its arguments here, makes one low-level call of `_lib.Sampler` (the device does the work per sample)
and finishes the pooled classifier with host arithmetic in float64.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .analysis import check_percentiles

TASK_CLS = _lib.TASK_CLS

# classification_report's result, K classes, N rows, S samples, Q = len(names) metric columns.  names: the columns, in the
# device's order; support [K] int64 = rows per class.  The pooled classifier argmax p_mean: confusion [K, K] int64 (row = the
# label, column = the prediction), metrics {name: value}, roc {k: (fpr, tpr, thresholds) or None}, p_mean [N, K] float64, p_correct
# [N] float64 = the share of the samples that give the row its label.  Over the samples: confusion_mean [K, K] float64,
# metric_mean {name: value}, metric_percentiles {p: {name: value}}, sample_metrics [S, Q] float32 (chain-major), sample_confusion
# [S, K, K] int32 or None; n_samples; n_distinct.  A dict by name holds a float for accuracy, balanced_accuracy, macro_f1 and
# macro_auc and a [K] float64 array for precision, recall, f1 and auc; what the labels leave undefined is NaN.
ClassificationReport = namedtuple("ClassificationReport", "names support confusion metrics roc p_mean p_correct confusion_mean "
                                                          "metric_mean metric_percentiles sample_metrics sample_confusion n_samples "
                                                          "n_distinct")

_SUMMARY = ("accuracy", "balanced_accuracy", "macro_f1", "macro_auc")
_PER_CLASS = ("precision", "recall", "f1", "auc")


def report_names(K, auc=True):
    """The metric columns of K classes, in the device's order: Q = 4 + 4 K names, or 3 + 3 K without the auc columns."""
    groups = _PER_CLASS if auc else _PER_CLASS[:3]
    return list(_SUMMARY if auc else _SUMMARY[:3]) + [f"{g}[{k}]" for g in groups for k in range(K)]


def confusion_matrix(y, pred, K):
    """conf[i, j] = rows with label i and prediction j -> [K, K] int64."""
    y, pred = np.asarray(y, dtype=np.int64), np.asarray(pred, dtype=np.int64)
    return np.bincount(y * K + pred, minlength=K * K).reshape(K, K).astype(np.int64)


def auc_pairs(scores, positive):
    """Twice the Mann-Whitney U statistic of the positives against the negatives, ties counted half: sum over (positive n,
    negative m) of 2 [s_n > s_m] + [s_n == s_m], an int, from the sorted scores and their runs of ties.  auc = it / (2 n_pos n_neg)."""
    s, pos = np.asarray(scores), np.asarray(positive, dtype=bool)
    order = np.argsort(s, kind="stable")
    s, pos = s[order], pos[order]
    new = np.ones(s.size, bool)
    new[1:] = s[1:] != s[:-1]
    run = np.cumsum(new) - 1                                                 # the run of ties of every sorted position
    neg_in_run = np.bincount(run, weights=~pos, minlength=run[-1] + 1 if s.size else 0).astype(np.int64)
    neg_below = np.cumsum(neg_in_run) - neg_in_run                           # negatives in the runs before
    return int(np.sum((2 * neg_below + neg_in_run)[run[pos]]))


def scores_from_confusion(conf, auc2=None):
    """The metric columns of one confusion matrix [K, K] (and, with auc2 [K] from auc_pairs, the auc columns) -> [Q] float64 in
    report_names' order.  Each is one division of integers; a mean over classes is the sum of those quotients in class order
    divided by their count.  precision of a never-predicted class is 0; recall and f1 of an absent class, auc of a class that
    holds no row or every row, and a mean with no class left are NaN."""
    conf = np.asarray(conf, dtype=np.int64)
    K, N = conf.shape[0], int(conf.sum())
    nk, col, hit = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    nan = float("nan")
    prec = [int(hit[k]) / int(col[k]) if col[k] > 0 else 0.0 for k in range(K)]
    rec = [int(hit[k]) / int(nk[k]) if nk[k] > 0 else nan for k in range(K)]
    f1 = [2 * int(hit[k]) / int(nk[k] + col[k]) if nk[k] > 0 else nan for k in range(K)]

    def mean(values):
        kept = [v for v in values if v == v]
        total = 0.0
        for v in kept:
            total += v
        return total / len(kept) if kept else nan
    head = [int(hit.sum()) / N if N else nan, mean(rec), mean(f1)]
    if auc2 is None:
        return np.array(head + prec + rec + f1, dtype=np.float64)
    au = [int(auc2[k]) / int(2 * nk[k] * (N - nk[k])) if 0 < nk[k] < N else nan for k in range(K)]
    return np.array(head + [mean(au)] + prec + rec + f1 + au, dtype=np.float64)


def roc_curve(scores, positive):
    """The ROC curve of one class against the rest: (fpr, tpr, thresholds), a point per distinct score, descending, after the
    point (0, 0) whose threshold is inf; a row counts as positive-predicted at threshold t when its score is >= t.  None when the
    class holds no row or every row.  The trapezoid area under it is auc_pairs / (2 n_pos n_neg)."""
    s, pos = np.asarray(scores, dtype=np.float64), np.asarray(positive, dtype=bool)
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        return None
    order = np.argsort(-s, kind="stable")
    s, pos = s[order], pos[order]
    last = np.flatnonzero(np.append(s[1:] != s[:-1], True))                  # the last position of every run of ties
    tp, fp = np.cumsum(pos)[last], np.cumsum(~pos)[last]
    return (np.concatenate([[0.0], fp / n_neg]), np.concatenate([[0.0], tp / n_pos]), np.concatenate([[np.inf], s[last]]))


def _undefined(support, n_rows, auc):
    """Which metric columns the labels leave undefined -> [Q] bool, in report_names' order."""
    nk = np.asarray(support)
    absent, unranked = nk == 0, (nk == 0) | (nk == n_rows)
    no = np.zeros(nk.size, bool)
    head = [False, bool(absent.all()), bool(absent.all())] + ([bool(unranked.all())] if auc else [])
    return np.concatenate([head, no, absent, absent] + ([unranked] if auc else []))


def _by_name(values, K, auc):
    """[..., Q] metric columns -> {name: float, or [..., K] array per class}."""
    v = np.asarray(values, dtype=np.float64)
    summary, groups = (_SUMMARY, _PER_CLASS) if auc else (_SUMMARY[:3], _PER_CLASS[:3])
    h = len(summary)
    out = {name: (float(v[k]) if v.ndim == 1 else v[..., k]) for k, name in enumerate(summary)}
    out.update({g: v[..., h + j * K:h + (j + 1) * K] for j, g in enumerate(groups)})
    return out


class ReportAnalysis:
    """classification_report(), for `ParallelTemperingBase` to inherit next to `PosteriorAnalysis`, whose row, sample-source and
    percentile helpers it uses.  It reads the constructor's attributes `task`, `topology` and `_sampler`."""

    def classification_report(self, data="test", *, percentiles=(5, 95), auc=True, burn_in=None, chains="all", thin=1, weights=None,
                              return_samples=False):
        """How well the classifier separates its classes, and how much that varies over the posterior, computed on the GPU
        (DESIGN.md section 26): the confusion matrix, per-class precision, recall and F1, and one-vs-rest ROC-AUC -- what one
        accuracy figure hides on an unbalanced problem.  Classification only.

        `data`: "train", "test" or rows whose first n_in + 1 columns are the inputs and the label.  Sample set, `chains`,
        `thin` and `weights` as in posterior_predictive; percentiles follow np.percentile(method="linear") exactly.  Every
        selected sample's net classifies every row (argmax of its probabilities, first index on a tie); its confusion counts
        and, per class, its Mann-Whitney count of the scores (ties half) are exact integers, and its metrics one division each.
        auc=False leaves the auc columns out; with them a call takes at most 16384 rows.

        -> ClassificationReport: names (the metric columns), support; of the pooled classifier argmax p_mean: confusion,
        metrics, roc[k] = (fpr, tpr, thresholds), p_mean, and p_correct (per row, the share of the samples that get it right);
        over the samples: confusion_mean, metric_mean, metric_percentiles[q], sample_metrics [n_samples, Q] (chain-major) and,
        with return_samples=True, sample_confusion [n_samples, K, K]; n_samples, n_distinct.  metrics, metric_mean and
        metric_percentiles[q] are dicts: accuracy, balanced_accuracy, macro_f1, macro_auc (floats), precision, recall, f1, auc
        ([K] arrays); recall / f1 of a class without rows, auc of a class with no or all rows are NaN and left out of the
        macro means."""
        self._need_sampler("classification_report")
        if self.task != TASK_CLS:
            raise ValueError("classification_report: a regression has no classes")
        rows = self._rows("data", data, target=True)
        pcts = check_percentiles(percentiles)
        I, K = int(self.topology[0]), int(self.topology[2])
        labels = np.asarray(self._host_rows(rows))[:, I]
        bad = np.flatnonzero(~((labels >= 0) & (labels < K) & (labels == np.floor(labels))))
        if bad.size:
            raise ValueError(f"class label {labels[bad[0]]} in row {int(bad[0])} is not an integer in [0, {K})")
        N, auc = labels.size, bool(auc)
        if auc and N > _lib.REPORT_MAX_AUC_ROWS:
            raise ValueError(f"auc: {N} rows, at most {_lib.REPORT_MAX_AUC_ROWS} per call; auc=False has no cap")
        kw, M = self._sample_source(weights, burn_in, chains, thin, count=True)
        spots, ranks = self._band_ranks(M, pcts)
        out = self._sampler.class_report(rows, ranks=ranks, auc=auc, sample_confusion=bool(return_samples), **kw)
        y = labels.astype(np.int64)
        support = np.bincount(y, minlength=K).astype(np.int64)
        undefined = _undefined(support, N, auc)

        def finish(values):
            v = np.array(values, dtype=np.float64)
            v[..., undefined] = np.nan
            return _by_name(v, K, auc)
        p_mean, S = out["p_mean"], out["n_samples"]
        confusion = confusion_matrix(y, np.argmax(p_mean, axis=1), K)
        auc2 = [auc_pairs(p_mean[:, k], y == k) for k in range(K)] if auc else None
        bands = self._bands(out["metric_order_stats"], pcts, spots, ranks) if ranks else {}
        sample_metrics = out["sample_metrics"]
        sample_metrics[:, undefined] = np.nan
        return ClassificationReport(
            names=report_names(K, auc), support=support, confusion=confusion,
            metrics=_by_name(scores_from_confusion(confusion, auc2), K, auc),
            roc={k: roc_curve(p_mean[:, k], y == k) for k in range(K)}, p_mean=p_mean, p_correct=out["p_correct"],
            confusion_mean=out["confusion_sum"] / float(S), metric_mean=finish(out["metric_mean"]),
            metric_percentiles={p: finish(v) for p, v in bands.items()}, sample_metrics=sample_metrics,
            sample_confusion=out["sample_confusion"], n_samples=S, n_distinct=out["n_distinct"])

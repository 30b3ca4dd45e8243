"""Reference for the classification report (ptnn_class_report / classification_report): float64 numpy, no device.  From the
outputs fx [U, N, K] of U distinct samples with integer counts on N rows with labels y: the confusion counts and the Mann-Whitney
counts of every sample (exact integers), the metric columns (one division each, a mean over classes summed in class order), and
their weighted mean and np.percentile bands over the expanded multiset.  The AUC integer is computed twice: the O(N^2) pair count
of the definition, and average ranks (argsort plus runs of ties)."""
import numpy as np

SUMMARY = ("accuracy", "balanced_accuracy", "macro_f1", "macro_auc")
PER_CLASS = ("precision", "recall", "f1", "auc")


def names(K, auc=True):
    return list(SUMMARY if auc else SUMMARY[:3]) + [f"{g}[{k}]" for g in (PER_CLASS if auc else PER_CLASS[:3]) for k in range(K)]


def confusion(p, y, K):
    """conf[i, j] = #{n: y_n = i, argmax_k p[n, k] = j}, first index on a tie.  p [N, K]."""
    pred = np.argmax(p, axis=1)
    conf = np.zeros((K, K), np.int64)
    for i, j in zip(y, pred):
        conf[int(i), int(j)] += 1
    return conf


def auc2_pairs(s, pos):
    """sum over (positive n, negative m) of 2 [s_n > s_m] + [s_n == s_m]: the definition, O(N^2)."""
    a, b = s[pos][:, None], s[~pos][None, :]
    return int(2 * np.sum(a > b) + np.sum(a == b))


def auc2_ranks(s, pos):
    """The same integer from average ranks: with r2 = twice the average 1-based rank of a score (an integer: the scores below it
    + the scores at or below it + 1), 2 U = sum over the positives of r2 - n_pos (n_pos + 1)."""
    srt = np.sort(s)
    r2 = np.searchsorted(srt, s, side="left") + np.searchsorted(srt, s, side="right") + 1
    n_pos = int(pos.sum())
    return int(r2[pos].sum()) - n_pos * (n_pos + 1)


def integers(fx, y, K, auc2=auc2_ranks):
    """conf [U, K, K] and auc2 [U, K] of outputs fx [U, N, K]."""
    y = np.asarray(y, dtype=np.int64)
    conf = np.stack([confusion(p, y, K) for p in fx])
    a2 = np.array([[auc2(p[:, k], y == k) for k in range(K)] for p in fx], dtype=np.int64).reshape(len(fx), K)
    return conf, a2


def metrics(conf, auc2=None):
    """The Q columns of one sample in float64, NaN where the labels leave a column undefined."""
    K, N = conf.shape[0], int(conf.sum())
    nan = float("nan")
    nk = [int(conf[k].sum()) for k in range(K)]
    col = [int(conf[:, k].sum()) for k in range(K)]
    hit = [int(conf[k, k]) for k in range(K)]
    prec = [hit[k] / col[k] if col[k] else 0.0 for k in range(K)]
    rec = [hit[k] / nk[k] if nk[k] else nan for k in range(K)]
    f1 = [(2 * hit[k]) / (nk[k] + col[k]) if nk[k] else nan for k in range(K)]

    def mean(v):
        kept = [x for x in v if not np.isnan(x)]
        t = 0.0
        for x in kept:
            t = t + x
        return t / len(kept) if kept else nan
    out = [sum(hit) / N, mean(rec), mean(f1)]
    if auc2 is None:
        return np.array(out + prec + rec + f1)
    au = [int(auc2[k]) / (2 * nk[k] * (N - nk[k])) if 0 < nk[k] < N else nan for k in range(K)]
    return np.array(out + [mean(au)] + prec + rec + f1 + au)


def report(fx, counts, y, K, auc=True, percentiles=()):
    """Everything per sample and over the expanded multiset.  fx [U, N, K]; counts [U] ints."""
    counts = np.asarray(counts, dtype=np.int64)
    conf, a2 = integers(fx, y, K)
    m = np.stack([metrics(conf[u], a2[u] if auc else None) for u in range(len(fx))])
    expanded = np.repeat(m, counts, axis=0)
    with np.errstate(invalid="ignore"):
        bands = {q: np.percentile(expanded.astype(np.float32).astype(np.float64), q, axis=0) for q in percentiles}
    return dict(conf=conf, auc2=a2, metrics=m, confusion_sum=(conf * counts[:, None, None]).sum(axis=0),
                metric_mean=expanded.astype(np.float32).astype(np.float64).mean(axis=0), bands=bands,
                sample_metrics=expanded.astype(np.float32), sample_confusion=np.repeat(conf, counts, axis=0).astype(np.int32))

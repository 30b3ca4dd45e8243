"""The cases on which ptnn_rank_convergence is compared with the float64 reference tests/rank_ref.py: shapes, input kinds, the
seed of every case and the rule for what a case may exempt.  tests/test_gpu_rank.py runs them on the device; tests/test_rank_cpu.py
checks, from the reference alone, that the seeds leave at most one truncation per case within rounding."""
import numpy as np

PROBS = (0.25, 0.9)
KINDS = ("ar1", "ties", "cauchy", "special")

# (1, 4, 1) .. (3, 4000, 2): the shapes every estimator test here uses.  The sort of a segment of S' = 2 C (n // 2) words runs in LDS
# alone up to 4096 words and takes global steps from 8192: S' = 4096 and 4104; one chain's 2h = 4096 and 4100 for the per-chain
# segments; (130, 4, 3) with 64 bins has more counters than the LDS histogram holds.  700, 256, 12000 .. are no powers of two.
GRID = [(1, 4, 1), (2, 5, 63), (7, 101, 65), (64, 4, 300), (3, 4000, 2), (4, 1024, 2), (4, 1026, 2), (1, 4096, 1), (1, 4100, 2),
        (130, 4, 3)]

DECIDED = 1e-9      # a truncation is compared only where the pair sum that decided it is at least this in size


def series(C, n, Q, seed):
    """Draws [C, n, Q] float64: AR(1) with phi from -0.5 to 0.999 over the quantities."""
    rng = np.random.default_rng(seed)
    phi = np.linspace(-0.5, 0.999, Q) if Q > 1 else np.array([0.6])
    y = np.empty((C, n, Q))
    y[:, 0] = rng.standard_normal((C, Q)) / np.sqrt(1 - phi ** 2)
    e = rng.standard_normal((C, n, Q))
    for i in range(1, n):
        y[:, i] = phi * y[:, i - 1] + e[:, i]
    return y + rng.standard_normal(Q) * 3


def draws(C, n, Q, kind, seed):
    """fp32 draws [C, n, Q] of one input kind.  ties: the series quantised to about ten levels, with runs of repeated rows (as
    rejected steps leave them).  special: quantity 0 constant, 1 constant within each chain, 2 with a NaN, 3 with +inf, 4 and on
    symmetric about their median (folded ties), as far as Q reaches, counted from the last quantity when Q < 5."""
    rng = np.random.default_rng(seed + 17)
    y = series(C, n, Q, seed)
    if kind == "ties":
        y = np.round(y * 1.5) / 1.5
        keep = rng.random((C, n)) < 0.4                                           # a row is new with probability 0.4
        keep[:, 0] = True
        src = np.maximum.accumulate(np.where(keep, np.arange(n), 0), axis=1)
        y = np.take_along_axis(y, src[:, :, None], axis=1)
    elif kind == "cauchy":
        y = rng.standard_cauchy((C, n, Q))
    elif kind == "special":
        special = ["const", "chain", "nan", "inf", "sym"]
        for q in range(Q):
            what = special[min(q, 4)] if Q >= 5 else special[(q + seed) % 5]
            if what == "const":
                y[:, :, q] = 1.25
            elif what == "chain":
                y[:, :, q] = np.arange(C)[:, None] * 0.5
            elif what == "nan":
                y[C // 2, n // 3, q] = np.nan
            elif what == "inf":
                y[C - 1, n - 1, q] = np.inf
            else:
                v = np.round(y[:, :, q] * 4) / 4                                   # multiples of 1/4, mirrored: exact in fp32
                h = n // 2
                v[:, n - h:] = -v[:, :h][:, ::-1]
                y[:, :, q] = v
    return y.astype(np.float32)


def case(C, n, Q, kind):
    """One case of GRID x KINDS -> (draws [C, n, Q] fp32, per_chain, bins): its seed, whether the per-chain figures are asked for,
    and the bin count (a bin per half rank where 64 bins allow it, so that the histogram holds the ranks)."""
    seed = C * 100003 + n * 7 + Q
    S = 2 * C * (n // 2)
    bins = 2 * S if 2 * S <= 64 else 64 if C == 130 else 20
    return draws(C, n, Q, kind, seed), C * Q <= 1024, bins


def undecided(want, per_chain):
    """The ESS comparisons a case leaves out, from the reference's deciding pair sums -> (dec [3 + len(PROBS), Q] over ess_bulk,
    ess_tail, ess_median and the quantile ESS, dec_chain [C, 3, Q] over ess_bulk_chain and the two indicators of ess_tail_chain, or
    None, exempt [Q]: the quantities with any comparison left out)."""
    dec = np.abs(np.nan_to_num(want["deciding"], nan=1.0)) < DECIDED              # bulk, the 0.05, 0.95 and 0.5 indicators, PROBS
    dec = np.stack([dec[0], dec[1] | dec[2], *dec[3:]])                            # as the figures: ess_tail is the smaller of two
    exempt, dc = dec.any(axis=0), None
    if per_chain:
        dc = np.abs(np.nan_to_num(want["deciding_chain"], nan=1.0)) < DECIDED
        exempt = exempt | dc.any(axis=(0, 1))
    return dec, dc, exempt

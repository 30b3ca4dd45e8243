"""Barrier vs pipelined swap cascade: windows on the critical path of one whole run, from its accept trace.
   cascade_sim.py [workload]                               -- runs the workload on the GPU and replays its trace
   cascade_sim.py [workload] --accept DIR/accept.npy       -- replays the trace `bench.py --dump-outputs DIR` wrote: needs no GPU
   What a persistent kernel gains that lets replica k start interval n+1 as soon as replicas 0 .. k+1 have handed off round n
   (swap_handoff) over the grid barrier, with the ring of D round slots (round n is posted only once every
   replica has started interval n-D+1) and, optionally, a round that costs --round-cost windows on either path."""
import os, sys, argparse, numpy as np
R_ = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R_)
import bench
ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="sunspot64")
ap.add_argument("--accept", metavar="FILE", help="accept.npy of bench.py --dump-outputs (cumulative accept counts [R, S])")
ap.add_argument("--slots", type=int, default=16, help="speculative slots per window (with --accept; describe() says it otherwise)")
ap.add_argument("--depths", default="2,3,4", help="ring depths to replay")
ap.add_argument("--round-cost", type=float, nargs=2, default=(0.0, 0.0), metavar=("BARRIER", "PIPELINED"), help="windows a round costs")
o = ap.parse_args()
wlname = o.workload
wl = dict(bench.WORKLOADS[wlname])
if o.accept:
    acc, slots = np.load(o.accept).astype(np.int64), o.slots
else:
    a = argparse.Namespace(waves=0, schedule=0, groups=0, bf16=False)
    train, test, _ = bench.load_data(wl["data"])
    lad = bench.Ladder(wl, a, train, test, 0, 1, 0)
    s = lad.s
    lad.whole_run()
    acc = s.traces(pos_w=False)["accept"].astype(np.int64)
    slots = s.describe()["slots_per_round"]
si = wl["si"]
flags = np.diff(acc, axis=1)[:, 1:]
n_int = flags.shape[1] // si
R = flags.shape[0]
rounds = np.zeros((n_int, R), dtype=np.int64)
for it in range(n_int):
    f = flags[:, 1 + it * si: 1 + (it + 1) * si]
    for k, row in enumerate(f):
        pos = n = 0
        while pos < row.shape[0]:
            hit = np.flatnonzero(row[pos:pos + slots])
            pos += (hit[0] + 1) if hit.size else slots
            n += 1
        rounds[it, k] = n
cb, cp = o.round_cost
barrier = (rounds.max(axis=1) + cb).sum()


def pipelined(depth):
    """Finish time of the last replica.  F[k]: replica k is through its interval; it starts the next one once 0 .. k+1 are through
    and -- ring of `depth` slots -- it may post round n only after everybody has started interval n - depth + 1."""
    F = np.zeros(R)
    starts = []                                          # starts[n]: the time the last replica took round n (started interval n+1)
    for it in range(n_int):
        post = F if depth is None or it < depth else np.maximum(F, starts[it - depth])
        pm = np.maximum.accumulate(post)                 # prefix max over posts
        start = np.empty(R)
        start[:-1] = pm[1:]                              # max over j <= k+1
        start[-1] = pm[-1]
        start = start + cp
        starts.append(start.max())
        F = start + rounds[it]
    return F.max()


print(f"{wlname}: slots {slots}, intervals {n_int}, mean windows {rounds.mean():.2f}, mean of max {rounds.max(axis=1).mean():.2f}")
print(f"slowest replica's index, bins of 8: {np.bincount(rounds.argmax(axis=1) // 8, minlength=(R + 7) // 8).tolist()}")
print(f"critical path in windows: barrier {barrier:.0f}, lower bound (busiest replica) {rounds.sum(axis=0).max()}")
free = pipelined(None)
print(f"  pipelined, unbounded buffering: {free:.0f} ({barrier / free:.3f}x)")
for d in (int(x) for x in o.depths.split(",")):
    t = pipelined(d)
    print(f"  pipelined, ring of {d}: {t:.0f} ({barrier / t:.3f}x)")
# even/odd or any other re-association is not allowed: the cascade is sequential in k (REG:694-759)

#!/usr/bin/env python3
"""A/B of the bandit grid posterior of the optimal arm on every prefix of N records (include/dpt_hip.h,
"Bayes posterior of the optimal action"), in one process.

Arm "kernel": ``dpt_hip.bandit_posterior`` (dpt_bandit_posterior: one workgroup walks a task's prefixes, the
weights and CDFs of its arms in LDS).  Arm "torch": the same definition restated in torch on the device, float64,
batched over the tasks and looping over t, recomputing only the pulled arm's weights between two rows as the
kernel does.  Beside them, untimed against each other: the numpy oracle tests/posterior_oracle.py on the CPU at
``--numpy_tasks`` tasks, extrapolated linearly in N (its work is independent per task).

Shapes (N, H, A, G): (1024, 500, 5, 1024), (1024, 100, 5, 256), (1024, 100, 20, 1024), Gaussian rewards of std
0.3 on uniformly random pulls.  All shapes are warmed up first; then per shape the two device arms run
``--rounds`` alternating rounds of ``--steps`` calls each; every round starts and ends in a device synchronise
and is timed with the host clock.  The spread of an arm is (max - min) / median of its round times: the
difference between runs of the same code, which any difference between the arms has to exceed.

Also timed (once, after a warm-up at 64 samples): ``train_fresh.bayes_floor`` for the 20,000 test samples of
``train_fresh.py --env bandit --envs 100000 --H 500 --dim 5 --var 0.3``, generator included.

Writes one JSON document (default profiles/posterior/ab.json).  Needs the GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [("N1024-H500-A5-G1024", 1024, 500, 5, 1024, 2), ("N1024-H100-A5-G256", 1024, 100, 5, 256, 5),
          ("N1024-H100-A20-G1024", 1024, 100, 20, 1024, 2)]  # name, N, H, A, G, default calls per timed round
VAR = 0.3


def summary(times, steps):
    per = [t / steps * 1e3 for t in times]
    med = statistics.median(per)
    return {"ms_per_call_rounds": [round(x, 3) for x in per], "ms_per_call_median": round(med, 3),
            "spread": round((max(per) - min(per)) / med, 4), "timed_calls": steps * len(times)}


def torch_posterior(acts, rews, A, var, G):
    """the header's Gaussian definition in torch: post (N, H + 1, A) float64"""
    N, H = acts.shape
    dev = acts.device
    x = (torch.arange(G, dtype=torch.float64, device=dev) + 0.5) / G
    rows = torch.arange(N, device=dev)

    def weights_cdf(n, s):  # (M,) each -> w, C (M, G)
        n, s = n[:, None], s[:, None]
        ll = -((n * x) * x - (2 * s) * x) / ((2 * var) * var)
        e = torch.exp(ll - ll.max(dim=-1, keepdim=True).values)
        w = e / e.sum(dim=-1, keepdim=True)
        return w, torch.cumsum(w, dim=-1) - w + w / 2

    def normalise(W, C):
        pre, suf = torch.ones_like(C), torch.ones_like(C)
        for a in range(1, A):
            pre[:, a] = pre[:, a - 1] * C[:, a - 1]
        for a in range(A - 2, -1, -1):
            suf[:, a] = suf[:, a + 1] * C[:, a + 1]
        u = (W * (pre * suf)).sum(dim=-1)
        return u / u.sum(dim=-1, keepdim=True)

    cnt = torch.zeros((N, A), dtype=torch.float64, device=dev)
    tot = torch.zeros((N, A), dtype=torch.float64, device=dev)
    w0, c0 = weights_cdf(cnt.reshape(-1), tot.reshape(-1))
    W, C = w0.reshape(N, A, G).clone(), c0.reshape(N, A, G).clone()
    post = torch.empty((N, H + 1, A), dtype=torch.float64, device=dev)
    post[:, 0] = normalise(W, C)
    for t in range(H):  # (every action of the timed records is in range)
        a = acts[:, t].long()
        cnt[rows, a] += 1.0
        tot[rows, a] += rews[:, t]
        W[rows, a], C[rows, a] = weights_cdf(cnt[rows, a], tot[rows, a])
        post[:, t + 1] = normalise(W, C)
    return post


class Shape:
    def __init__(self, N, H, A, G):
        import dpt_hip
        dev = dpt_hip.device()
        self.N, self.H, self.A, self.G = N, H, A, G
        means = torch.rand((N, A), dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(H + A))
        probs = torch.full((N, A), 1.0 / A, dtype=torch.float64, device=dev)
        self.acts, self.rews = dpt_hip.rollin_bandit(means, probs, H, VAR, seed=H + A)

    def kernel(self):
        import dpt_hip
        return dpt_hip.bandit_posterior(self.acts, self.rews, self.A, VAR, dpt_hip.BANDIT_GAUSSIAN, grid=self.G)

    def torch(self):
        return torch_posterior(self.acts, self.rews, self.A, VAR, self.G)


def run_shape(name, shape, steps, args):
    import posterior_oracle as PO
    arms = {"kernel": shape.kernel, "torch": shape.torch}
    times = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[a].append(time.perf_counter() - t0)
    out = {a: summary(t, steps) for a, t in times.items()}
    out.update(N=shape.N, H=shape.H, A=shape.A, G=shape.G)
    a, b = out["kernel"]["ms_per_call_median"], out["torch"]["ms_per_call_median"]
    out["torch_over_kernel"] = round(b / a, 2)
    lo = min(a, b) * (1 + max(out["kernel"]["spread"], out["torch"]["spread"]))
    out["difference_exceeds_both_spreads"] = bool(max(a, b) > lo)
    # agreement, untimed: the two device arms on every task, the numpy oracle on the first few
    got, ref = shape.kernel(), shape.torch()
    out["max_abs_kernel_minus_torch"] = float((got - ref).abs().max())
    k = min(args.numpy_tasks, shape.N)
    acts, rews = shape.acts[:k].cpu().numpy(), shape.rews[:k].cpu().numpy()
    t0 = time.perf_counter()
    oracle = PO.bandit_posterior(acts, rews, shape.A, VAR, PO.GAUSSIAN, shape.G)
    dt = time.perf_counter() - t0
    out["numpy"] = {"tasks": k, "seconds": round(dt, 3), "extrapolated_seconds_for_N": round(dt * shape.N / k, 1),
                    "extrapolation": "linear in N (the oracle's work is independent per task)",
                    "max_abs_kernel_minus_numpy": float(np.abs(got[:k].cpu().numpy() - oracle).max())}
    print(name, json.dumps(out), flush=True)
    return out


def floor_timing():
    """train_fresh.bayes_floor on the README's 100,000-env bandit command: 20,000 test samples, H 500, 5 arms"""
    import dpt_hip
    import train_fresh
    env = dpt_hip.FreshEnv.bandit(5, 500, 0.3, "uniform")
    key = train_fresh.generator_key(1, "test")
    train_fresh.bayes_floor(env, key, 64, 500)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    floor = train_fresh.bayes_floor(env, key, 20000, 500)
    dt = time.perf_counter() - t0
    return {"command": "train_fresh.py --env bandit --envs 100000 --H 500 --dim 5 --var 0.3 --seed 1 --bayes_floor",
            "test_samples": 20000, "H": 500, "A": 5, "G": dpt_hip.posterior_grid(0.3, 500), "seconds": round(dt, 3),
            "bayes_floor": floor}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="calls per timed round (0: the shape's default)")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--numpy_tasks", type=int, default=8, help="tasks of the CPU oracle's subsample")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--no_floor", action="store_true", help="skip the --bayes_floor timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posterior_ab.py measures on the GPU; none is visible")
    want = set(filter(None, args.shapes.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "var": VAR, "rewards": "gaussian", "rounds": args.rounds,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms; "
                     "every shape warmed up (one call per arm) before the first timed round",
           "shapes": {}}
    shapes = [(name, Shape(N, H, A, G), args.steps or steps) for name, N, H, A, G, steps in SHAPES
              if not want or name in want]
    for _, shape, _ in shapes:  # warm every shape up first
        shape.kernel()
        shape.torch()
    torch.cuda.synchronize()
    for name, shape, steps in shapes:
        res["shapes"][name] = run_shape(name, shape, steps, args)
    if not args.no_floor:
        res["bayes_floor"] = floor_timing()
        print("bayes_floor", json.dumps(res["bayes_floor"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

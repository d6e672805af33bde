#!/usr/bin/env python3
"""A/B of the linear bandit's Bayes posterior of the optimal arm at lin_d = 2 on every prefix of N records
(include/dpt_hip.h, "Linear bandit, lin_d = 2"), in one process.

Arm "kernel": ``dpt_hip.linear_posterior`` (dpt_linear_posterior: one workgroup walks a task's prefixes, every
thread walks the upper envelope along its rays).  Arm "torch": the same definition restated in torch on the
device, float64, in its pairwise form, batched over the tasks (in slices that keep a (n, K, K, G) tensor at
2^28 elements) and looping over t; the prior and the kept arms come from the numpy oracle, outside the timing.
Beside them, untimed against each other: the numpy oracle tests/linear_posterior_oracle.py on the CPU at
``--numpy_tasks`` tasks, extrapolated linearly in N (its work is independent per task).

Shapes (N, H, A): (1024, 200, 10), the reference's run_linear_bandit.sh, and (1024, 1000, 20), both at the
default G; collect_data.py's arms, reward std 0.3, the records the device generator's Thompson rollin.  All shapes
are warmed up first; then per shape the two device arms run ``--rounds`` alternating rounds of ``--steps`` calls
each; every round starts and ends in a device synchronise and is timed with the host clock.  The spread of an
arm is (max - min) / median of its round times: the difference between runs of the same code, which any
difference between the arms has to exceed.

Also timed (once, after a warm-up at 64 samples): ``train_fresh.bayes_floor`` for the 20,000 test samples of
``train_fresh.py --env linear_bandit --data_type thompson --envs 100000 --H 1000 --dim 20 --lin_d 2 --var 0.3``,
generator included.

Writes one JSON document (default profiles/posterior_linear/ab.json).  Needs the GPU: there is no CPU fallback.
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

SHAPES = [("N1024-H200-A10", 1024, 200, 10, 1), ("N1024-H1000-A20", 1024, 1000, 20, 1)]  # name, N, H, A, calls per round
VAR = 0.3
TWO_PI = 6.283185307179586


def summary(times, steps):
    per = [t / steps * 1e3 for t in times]
    med = statistics.median(per)
    return {"ms_per_call_rounds": [round(x, 3) for x in per], "ms_per_call_median": round(med, 3),
            "spread": round((max(per) - min(per)) / med, 4), "timed_calls": steps * len(times)}


def torch_posterior(arms, keep, prior, acts, rews, var, G):
    """the header's definition in torch, pairwise form: post (N, H + 1, A) float64; ``keep`` the indices of the
    arms whose prior is not 0 (every action of the timed records is in range)"""
    N, H = acts.shape
    A, K = arms.shape[0], keep.numel()
    dev = acts.device
    phi = (TWO_PI * (torch.arange(G, dtype=torch.float64, device=dev) + 0.5)) / G
    c, s = torch.cos(phi), torch.sin(phi)
    xk = arms[keep]
    idx = torch.arange(K, device=dev)
    lower = (idx[None, :] < idx[:, None])[None, :, :, None]  # b < a
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    v2 = var * var
    post = torch.zeros((N, H + 1, A), dtype=torch.float64, device=dev)
    post[:, 0] = prior
    step = max(1, (1 << 28) // (K * K * G))
    for n0 in range(0, N, step):
        a_, r_ = acts[n0:n0 + step].long(), rews[n0:n0 + step]
        n = a_.shape[0]
        st = torch.zeros((n, 5), dtype=torch.float64, device=dev)
        for t in range(H):
            x, r = arms[a_[:, t]], r_[:, t]
            st = st + torch.stack([(x[:, 0] * x[:, 0]) / v2, (x[:, 0] * x[:, 1]) / v2, (x[:, 1] * x[:, 1]) / v2,
                                   (r * x[:, 0]) / v2, (r * x[:, 1]) / v2], 1)
            l00, l01, l11 = 2.0 + st[:, 0], st[:, 1], 2.0 + st[:, 2]
            det = l00 * l11 - l01 * l01
            s00, s01, s11 = l11 / det, -(l01 / det), l00 / det
            m0, m1 = s00 * st[:, 3] + s01 * st[:, 4], s01 * st[:, 3] + s11 * st[:, 4]
            L00 = torch.sqrt(s00)
            L10, L11 = s01 / L00, 1.0 / torch.sqrt(l11)
            alpha = xk[:, 0] * m0[:, None] + xk[:, 1] * m1[:, None]                         # (n, K)
            xl0, xl1 = xk[:, 0] * L00[:, None] + xk[:, 1] * L10[:, None], xk[:, 1] * L11[:, None]
            beta = xl0[:, :, None] * c + xl1[:, :, None] * s                                # (n, K, G)
            db = beta[:, :, None, :] - beta[:, None, :, :]
            da = (alpha[:, None, :] - alpha[:, :, None])[..., None]
            q = da / db
            lo = torch.where(db > 0, q, -inf).amax(2).clamp_min(0.0)
            hi = torch.where(db < 0, q, inf).amin(2)
            lost = ((db == 0) & ((da > 0) | ((da == 0) & lower))).any(2)
            mass = torch.exp(-(lo * lo) / 2.0) - torch.exp(-(hi * hi) / 2.0)
            u = torch.where((hi <= lo) | lost, torch.zeros_like(mass), mass).sum(-1)       # (n, K)
            post[n0:n0 + n, t + 1, keep] = u / u.sum(-1, keepdim=True)
    return post


class Shape:
    def __init__(self, N, H, A):
        import dpt_hip
        import linear_posterior_oracle as LO
        dev = dpt_hip.device()
        self.N, self.H, self.A, self.G = N, H, A, dpt_hip.linear_posterior_grid()
        self.arms_np = LO.reference_arms(A)
        prior = LO.prior(self.arms_np)
        self.arms = torch.as_tensor(self.arms_np, dtype=torch.float64, device=dev)
        self.prior = torch.as_tensor(prior, dtype=torch.float64, device=dev)
        self.keep = torch.as_tensor(np.nonzero(prior > 0)[0], device=dev)
        env = dpt_hip.FreshEnv.linear_bandit(self.arms_np, H, VAR, "thompson")
        tok = dpt_hip.fresh_batch(env, 1000 + H + A, 0, N, outputs=False)["tokens"]
        self.acts = tok[:, 1:, 1:1 + A].argmax(dim=-1).to(torch.int32).contiguous()
        self.rews = tok[:, 1:, 2 + A].to(torch.float64).contiguous()

    def kernel(self):
        import dpt_hip
        return dpt_hip.linear_posterior(self.arms, self.acts, self.rews, VAR, grid=self.G)

    def torch(self):
        return torch_posterior(self.arms, self.keep, self.prior, self.acts, self.rews, VAR, self.G)


def run_shape(name, shape, steps, args):
    import linear_posterior_oracle as LO
    arms = {"kernel": shape.kernel, "torch": shape.torch}
    times, last = {a: [] for a in arms}, {}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                last[a] = fn()
            torch.cuda.synchronize()
            times[a].append(time.perf_counter() - t0)
    out = {a: summary(t, steps) for a, t in times.items()}
    out.update(N=shape.N, H=shape.H, A=shape.A, G=shape.G, kept_arms=int(shape.keep.numel()))
    a, b = out["kernel"]["ms_per_call_median"], out["torch"]["ms_per_call_median"]
    out["torch_over_kernel"] = round(b / a, 2)
    lo = min(a, b) * (1 + max(out["kernel"]["spread"], out["torch"]["spread"]))
    out["difference_exceeds_both_spreads"] = bool(max(a, b) > lo)
    # agreement: the two device arms' last timed results on every task, the numpy oracle on the first few
    got, ref = last["kernel"], last["torch"]
    out["max_abs_kernel_minus_torch"] = float((got - ref).abs().max())
    k = min(args.numpy_tasks, shape.N)
    acts, rews = shape.acts[:k].cpu().numpy(), shape.rews[:k].cpu().numpy()
    t0 = time.perf_counter()
    oracle = LO.linear_posterior(shape.arms_np, acts, rews, VAR, shape.G)
    dt = time.perf_counter() - t0
    out["numpy"] = {"tasks": k, "seconds": round(dt, 3), "extrapolated_seconds_for_N": round(dt * shape.N / k, 1),
                    "extrapolation": "linear in N (the oracle's work is independent per task)",
                    "max_abs_kernel_minus_numpy": float(np.abs(got[:k].cpu().numpy() - oracle).max())}
    print(name, json.dumps(out), flush=True)
    return out


def floor_timing():
    """train_fresh.bayes_floor on the README's 100,000-env linear command: 20,000 test samples, H 1000, 20 arms"""
    import dpt_hip
    import linear_posterior_oracle as LO
    import train_fresh
    env = dpt_hip.FreshEnv.linear_bandit(LO.reference_arms(20), 1000, VAR, "thompson")
    key = train_fresh.generator_key(1, "test")
    train_fresh.bayes_floor(env, key, 64, 1000)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    floor = train_fresh.bayes_floor(env, key, 20000, 1000)
    dt = time.perf_counter() - t0
    return {"command": "train_fresh.py --env linear_bandit --data_type thompson --envs 100000 --H 1000 --dim 20 --lin_d 2 "
                       "--var 0.3 --seed 1 --bayes_floor",
            "test_samples": 20000, "H": 1000, "A": 20, "G": dpt_hip.linear_posterior_grid(), "seconds": round(dt, 3),
            "bayes_floor": floor}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="calls per timed round (0: the shape's default)")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds per arm")
    ap.add_argument("--numpy_tasks", type=int, default=2, help="tasks of the CPU oracle's subsample")
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--no_floor", action="store_true", help="skip the --bayes_floor timing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_linear", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posterior_linear_ab.py measures on the GPU; none is visible")
    want = set(filter(None, args.shapes.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "var": VAR, "rollin": "thompson", "rounds": args.rounds,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms; "
                     "every shape warmed up (one call per arm) before the first timed round",
           "shapes": {}}
    shapes = [(name, Shape(N, H, A), args.steps or steps) for name, N, H, A, steps in SHAPES if not want or name in want]
    for _, shape, _ in shapes:  # warm every shape up first
        shape.kernel()
        shape.torch()
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():  # after every part: a run cut short leaves what it measured
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not args.no_floor:
        res["bayes_floor"] = floor_timing()
        print("bayes_floor", json.dumps(res["bayes_floor"]), flush=True)
        write()
    for name, shape, steps in shapes:
        res["shapes"][name] = run_shape(name, shape, steps, args)
        write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()

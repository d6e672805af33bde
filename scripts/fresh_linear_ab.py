#!/usr/bin/env python3
"""A/B of the linear bandit's pretraining step: the parent commit's ``Trainer.step`` on a resident dataset
against ``FreshTrainer.step`` on ``FreshEnv.linear_bandit`` (dpt_fresh_linear_step: the batch, Thompson rollin
included, generated on the device), each arm in its own process.  Protocol as scripts/fresh_step_ab.py.

Arm "resident": ``Trainer.step`` on the library given first -- the parent commit's build (``make -C csrc`` in a
checkout of the parent, copied to dpt_hip/libdpt_hip_parent.so) -- on a resident dataset of the linear
bandit's shapes.  Arms "thompson" and "uniform": ``FreshTrainer.step`` with that rollin on the library given
second (default libdpt_hip.so).  Shape: BASELINE config 4, 20 arms, 2 features, window 1001, batch 64, 4
layers, width 32.  Per arm a warm-up, then ``--rounds`` alternating rounds of ``--steps`` steps, every round
between device synchronisations on the host clock; the spread of an arm is (max - min) / median of its rounds.

The fresh arms' processes also time dpt_fresh_linear_batch alone (device events around ``--gen_reps`` calls
of 64 samples after a warm-up) at that shape and at 5 arms, H 500, both rollins.

Writes ab.json under --out (default profiles/fresh_linear).  ``--collect``: also the wall time of
collect_data.py --env linear_bandit --envs 10000 --H 1000 --dim 20 --var 0.3 plus train.py's load and upload
of the training set, the phase the fresh step removes (ungated).  Needs the GPU.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "decision-pretrained-transformer_amd")
sys.path[:0] = [PKG, os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402

from ab_lib import step_data  # noqa: E402

A, D, H, VAR = 20, 2, 1000, 0.3
GEN_SHAPES = [("A20_H1000", 20, 1000), ("A5_H500", 5, 500)]
ARMS = ("resident", "thompson", "uniform")


def arms_of(n_arms, d):
    return np.random.RandomState(seed=1234).normal(size=(n_arms, d)) / np.sqrt(d)  # collect_data.py's


def generator_ms(rollin, n_arms, horizon, batch, reps):
    """ms per dpt_fresh_linear_batch of ``batch`` samples, device events around ``reps`` calls"""
    import torch
    import dpt_hip
    env = dpt_hip.FreshEnv.linear_bandit(arms_of(n_arms, D), horizon, VAR, rollin)
    for i in range(3):
        dpt_hip.fresh_batch(env, 1, i * batch, batch, outputs=False)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        dpt_hip.fresh_batch(env, 1, (3 + i) * batch, batch, outputs=False)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def child(lib, arm, args):
    """one arm on one library: seconds of one round, and the generator alone in the fresh arms"""
    from dpt_hip import _lib
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.__file__), lib)
    import torch
    import dpt_hip
    import dpt_hip.train as tr
    from models.net import Transformer
    res = {"lib": lib, "arm": arm, "device": torch.cuda.get_device_name(0)}
    B = args.batch
    torch.manual_seed(H)
    rs = np.random.RandomState(H)
    model = Transformer(dict(horizon=H, state_dim=1, action_dim=A, n_layer=args.layer, n_embd=args.embd, n_head=1,
                             dropout=0.0, test=False)).cuda().train()
    if arm == "resident":
        t = tr.Trainer(model, lr=1e-3, weight_decay=1e-4)
        dd = t.device_data(step_data(rs, 4 * B, H, 1, A))
        plans = [torch.from_numpy(rs.randint(0, 4 * B, B)) for _ in range(args.steps)]  # host index batches

        def run(k):
            for i in range(k):
                t.step(dd, plans[i % len(plans)])
            return t.read_loss()
    else:
        env = dpt_hip.FreshEnv.linear_bandit(arms_of(A, D), H, VAR, arm)
        t = tr.FreshTrainer(model, env, lr=1e-3, weight_decay=1e-4, seed=H)

        def run(k):
            for _ in range(k):
                t.step(B)
            return t.read_loss()
    run(args.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    torch.cuda.synchronize()
    res["seconds"] = time.perf_counter() - t0
    if arm != "resident":
        res["generator_ms"] = {name: generator_ms(arm, n_arms, horizon, B, args.gen_reps)
                               for name, n_arms, horizon in GEN_SHAPES}
    print(json.dumps(res))


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_step_rounds": [round(x, 4) for x in per_step], "ms_per_step_median": round(med, 4),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_steps": steps * len(times)}


def collect_phase(workdir):
    """wall seconds of the phase the fresh step removes: collect_data.py for 10,000 linear-bandit tasks of
    horizon 1000 with 20 arms, then train.py's load of the training set (unpickle, stack, upload)"""
    flags = ["--env", "linear_bandit", "--envs", "10000", "--H", str(H), "--dim", str(A), "--lin_d", str(D),
             "--var", str(VAR)]
    os.makedirs(workdir, exist_ok=True)
    t0 = time.perf_counter()
    subprocess.run([sys.executable, os.path.join(PKG, "collect_data.py"), *flags], cwd=workdir, check=True,
                   capture_output=True, timeout=900)
    collect = time.perf_counter() - t0
    code = ("import sys, time; sys.path.insert(0, %r); import torch; from dataset import Dataset; "
            "from dpt_hip.train import DeviceData; from utils import build_linear_bandit_data_filename as f; "
            "cfg = {'n_hists': 1, 'n_samples': 1, 'horizon': %d, 'dim': %d, 'lin_d': %d, 'var': %r, 'cov': 0.0}; "
            "t0 = time.perf_counter(); "
            "d = Dataset(f('linear_bandit', 10000, cfg, mode=0), {'horizon': %d, 'state_dim': 1, 'action_dim': %d, "
            "'shuffle': False, 'store_gpu': True}); DeviceData(d); torch.cuda.synchronize(); "
            "print(time.perf_counter() - t0)" % (PKG, H, A, D, VAR, H, A))
    cp = subprocess.run([sys.executable, "-c", code], cwd=workdir, check=True, capture_output=True, text=True,
                        timeout=600)
    return {"command": "collect_data.py " + " ".join(flags), "collect_seconds": round(collect, 2),
            "load_train_set_seconds": round(float(cp.stdout.strip().splitlines()[-1]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=["libdpt_hip_parent.so", "libdpt_hip.so"],
                    help="the resident arm's library (the parent build) and the fresh arms', file names in dpt_hip/")
    ap.add_argument("--steps", type=int, default=200, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--gen_reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fresh_linear"))
    ap.add_argument("--collect", default="", help="a scratch directory: also time the collect phase there")
    ap.add_argument("--child", nargs=2, metavar=("LIB", "ARM"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args)
    if len(args.libs) != 2:
        raise SystemExit("two libraries: the parent build (resident arm) and this build (fresh arms)")
    libs = {"resident": args.libs[0], "thompson": args.libs[1], "uniform": args.libs[1]}
    times = {a: [] for a in ARMS}
    gen = {a: {name: [] for name, *_ in GEN_SHAPES} for a in ARMS[1:]}
    device = None
    for rnd in range(args.rounds):
        for arm in ARMS:
            cp = subprocess.run([sys.executable, __file__, "--child", libs[arm], arm, "--steps", str(args.steps),
                                 "--warmup", str(args.warmup), "--batch", str(args.batch), "--layer",
                                 str(args.layer), "--embd", str(args.embd), "--gen_reps", str(args.gen_reps)],
                                capture_output=True, text=True, timeout=600)
            if cp.returncode:
                sys.exit(f"{libs[arm]} ({arm}): child failed ({cp.returncode})\n{cp.stderr[-3000:]}")
            d = json.loads(cp.stdout.strip().splitlines()[-1])
            device = d["device"]
            times[arm].append(d["seconds"])
            for name, ms in d.get("generator_ms", {}).items():
                gen[arm][name].append(ms)
            print(f"round {rnd} {arm} {libs[arm]}: {d['seconds']:.4f} s {d.get('generator_ms', '')}", file=sys.stderr,
                  flush=True)
    res = {"device": device, "arms": A, "lin_d": D, "window": 1 + H, "var": VAR, "batch": args.batch,
           "n_layer": args.layer, "n_embd": args.embd, "steps_per_round": args.steps, "rounds": args.rounds,
           "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms, "
                     "one process per round and arm; the generator alone: device events around gen_reps calls",
           "libs": libs}
    res["step"] = {a: summary(times[a], args.steps) for a in ARMS}
    for a in ARMS[1:]:
        ratio = res["step"][a]["ms_per_step_median"] / res["step"]["resident"]["ms_per_step_median"]
        margin = max(res["step"]["resident"]["spread"], res["step"][a]["spread"])
        res["step"][a]["over_resident"] = round(ratio, 4)
        res["step"][a]["within_larger_spread"] = bool(ratio - 1 <= margin)
    res["generator_alone_ms_per_batch"] = {
        a: {name: {"rounds": [round(x, 4) for x in v], "median": round(statistics.median(v), 4)}
            for name, v in gen[a].items()} for a in gen}
    if args.collect:
        res["collect_phase"] = collect_phase(args.collect)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

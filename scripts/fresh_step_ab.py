#!/usr/bin/env python3
"""A/B of the pretraining step: the parent commit's ``Trainer.step`` on a resident dataset against
``FreshTrainer.step`` (dpt_fresh_step: the batch generated on the device), each arm in its own process.

Arm "resident": ``Trainer.step`` (dpt_train_step: the batch gathered from the resident dataset by a fresh
index batch) on the library given first -- the parent commit's build, e.g. ``make -C csrc`` in a checkout of
the parent, copied to dpt_hip/libdpt_hip_parent.so.  Arm "fresh": ``FreshTrainer.step`` on the library given
second (default libdpt_hip.so).  Shapes: batch 64, 4 layers, width 32, window 501 with 5 arms and window 101
DarkRoom, the two shapes of profiles/train_step/ab.json.  Protocol as scripts/train_step_ab.py: per shape
both arms warm up, then ``--rounds`` alternating rounds of ``--steps`` steps, every round between device
synchronisations on the host clock; the spread of an arm is (max - min) / median of its rounds.

The resident arm's process also digests ``Trainer.step`` / ``eval_loss`` on a small resident dataset
(``resident_digests``: sha1 over blob, m, v and the loss); both libraries must agree, and
tests/test_gpu_fresh_step.py holds later builds to the parent's column.

Writes ab.json and digests.txt under --out (default profiles/fresh_step).  ``--collect``: also the wall
time of collect_data.py --env bandit --envs 10000 --H 500 --dim 5 --var 0.3 plus train.py's dataset load
and upload, the phase the fresh step removes (ungated).  Needs the GPU.
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

from ab_lib import sha, step_data  # noqa: E402

SHAPES = [("bandit_T501", "bandit", 5, 500), ("darkroom_T101", "darkroom", 10, 100)]  # name, kind, dim, H


def resident_digests():
    """{case: sha1} of Trainer.step (6 samples, 4 with a context permutation, 6) + eval_loss on a resident
    dataset of 12 samples, horizon 8, 5 arms: widths 32 and 18, dropout 0 and 0.1 with the seeds passed in."""
    import torch
    import dpt_hip.train as tr
    from models.net import Transformer
    out, H, A = {}, 8, 5
    for E in (32, 18):
        for p in (0.0, 0.1):
            rs = np.random.RandomState(300 + E)
            torch.manual_seed(E)
            model = Transformer(dict(horizon=H, state_dim=1, action_dim=A, n_layer=2, n_embd=E, n_head=1, dropout=p,
                                     test=False)).cuda().train()
            data = step_data(rs, 12, H, 1, A)
            perm = np.stack([rs.permutation(H) for _ in range(4)])
            t = tr.Trainer(model, lr=1e-3)
            dd = t.device_data(data)
            t._run(True, dd, np.arange(0, 6), None, seed=21)
            t._run(True, dd, np.arange(6, 10), perm, seed=22)
            t._run(True, dd, np.arange(3, 9), None, seed=23)
            t._run(False, dd, np.arange(1, 6), None, seed=24)
            out[f"Trainer E{E} drop{p} steps 6,4p,6 + eval"] = sha(t.blob, t.m, t.v, t.loss, torch.tensor([t.steps]))
    return out


def make_env(kind, dim, H):
    import dpt_hip
    if kind == "bandit":
        return dpt_hip.FreshEnv.bandit(dim, H, 0.3, "uniform")
    goals = np.array([[(j, i) for i in range(dim)] for j in range(dim)]).reshape(-1, 2)
    return dpt_hip.FreshEnv.darkroom(dim, H, goals)


def child(lib, arm, args):
    """one arm on one library: {shape: seconds per round}, and the digests in the resident arm"""
    from dpt_hip import _lib
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.__file__), lib)
    import torch
    import dpt_hip.train as tr
    from models.net import Transformer
    res = {"lib": lib, "arm": arm, "device": torch.cuda.get_device_name(0), "seconds": {},
           "digests": resident_digests()}
    B = args.batch
    for name, kind, dim, H in SHAPES:
        sd, A = (1, dim) if kind == "bandit" else (2, 5)
        torch.manual_seed(H)
        rs = np.random.RandomState(H)
        model = Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=args.layer, n_embd=args.embd,
                                 n_head=1, dropout=0.0, test=False)).cuda().train()
        if arm == "resident":
            t = tr.Trainer(model, lr=1e-3, weight_decay=1e-4)
            dd = t.device_data(step_data(rs, 4 * B, H, sd, A))
            plans = [torch.from_numpy(rs.randint(0, 4 * B, B)) for _ in range(args.steps)]  # host index batches

            def run(k, i0=0):
                for i in range(k):
                    t.step(dd, plans[(i0 + i) % len(plans)])
                return t.read_loss()
        else:
            t = tr.FreshTrainer(model, make_env(kind, dim, H), lr=1e-3, weight_decay=1e-4, seed=H)

            def run(k, i0=0):
                for _ in range(k):
                    t.step(B)
                return t.read_loss()
        run(args.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(args.steps)
        torch.cuda.synchronize()
        res["seconds"][name] = time.perf_counter() - t0
    print(json.dumps(res))


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_step_rounds": [round(x, 4) for x in per_step], "ms_per_step_median": round(med, 4),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_steps": steps * len(times)}


def collect_phase(workdir):
    """wall seconds of the phase the fresh step removes: collect_data.py for 10,000 bandit tasks of horizon
    500, then train.py's load of the training set (unpickle, stack, upload)"""
    flags = ["--env", "bandit", "--envs", "10000", "--H", "500", "--dim", "5", "--var", "0.3"]
    os.makedirs(workdir, exist_ok=True)
    t0 = time.perf_counter()
    subprocess.run([sys.executable, os.path.join(PKG, "collect_data.py"), *flags], cwd=workdir, check=True,
                   capture_output=True, timeout=600)
    collect = time.perf_counter() - t0
    code = ("import sys, time; sys.path.insert(0, %r); import torch; from dataset import Dataset; "
            "from dpt_hip.train import DeviceData; from utils import build_bandit_data_filename as f; "
            "cfg = {'n_hists': 1, 'n_samples': 1, 'horizon': 500, 'dim': 5, 'var': 0.3, 'cov': 0.0, "
            "'type': 'uniform'}; "
            "t0 = time.perf_counter(); "
            "d = Dataset(f('bandit', 10000, cfg, mode=0), {'horizon': 500, 'state_dim': 1, 'action_dim': 5, "
            "'shuffle': False, 'store_gpu': True}); DeviceData(d); torch.cuda.synchronize(); "
            "print(time.perf_counter() - t0)" % PKG)
    cp = subprocess.run([sys.executable, "-c", code], cwd=workdir, check=True, capture_output=True, text=True,
                        timeout=300)
    return {"command": "collect_data.py " + " ".join(flags), "collect_seconds": round(collect, 2),
            "load_train_set_seconds": round(float(cp.stdout.strip().splitlines()[-1]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=["libdpt_hip_parent.so", "libdpt_hip.so"],
                    help="the resident arm's library (the parent build) and the fresh arm's, file names in dpt_hip/")
    ap.add_argument("--steps", type=int, default=200, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fresh_step"))
    ap.add_argument("--collect", default="", help="a scratch directory: also time the collect phase there")
    ap.add_argument("--child", nargs=2, metavar=("LIB", "ARM"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args)
    if len(args.libs) != 2:
        raise SystemExit("two libraries: the parent build (resident arm) and this build (fresh arm)")
    arms = {"resident": args.libs[0], "fresh": args.libs[1]}
    times = {a: {name: [] for name, *_ in SHAPES} for a in arms}
    digests, device = {}, None
    for rnd in range(args.rounds):
        for arm, lib in arms.items():
            cp = subprocess.run([sys.executable, __file__, "--child", lib, arm, "--steps", str(args.steps),
                                 "--warmup", str(args.warmup), "--batch", str(args.batch), "--layer",
                                 str(args.layer), "--embd", str(args.embd)], capture_output=True, text=True,
                                timeout=600)
            if cp.returncode:
                sys.exit(f"{lib} ({arm}): child failed ({cp.returncode})\n{cp.stderr[-3000:]}")
            d = json.loads(cp.stdout.strip().splitlines()[-1])
            device = d["device"]
            for name, s in d["seconds"].items():
                times[arm][name].append(s)
            if digests.setdefault(lib, d["digests"]) != d["digests"]:
                sys.exit(f"{lib}: the digests differ from round to round")
            print(f"round {rnd} {arm} {lib}: {d['seconds']}", file=sys.stderr, flush=True)
    res = {"device": device, "batch": args.batch, "n_layer": args.layer, "n_embd": args.embd,
           "steps_per_round": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms, "
                     "one process per round and arm",
           "libs": arms, "shapes": {}}
    for name, kind, dim, H in SHAPES:
        out = {a: summary(times[a][name], args.steps) for a in arms}
        out["window"] = 1 + H
        out["fresh_over_resident"] = round(out["fresh"]["ms_per_step_median"]
                                           / out["resident"]["ms_per_step_median"], 4)
        margin = max(out["resident"]["spread"], out["fresh"]["spread"])
        out["within_larger_spread"] = bool(out["fresh_over_resident"] - 1 <= margin)
        res["shapes"][name] = out
    a, b = (digests[lib] for lib in args.libs)
    res["digests_equal"] = a == b
    if args.collect:
        res["collect_phase"] = collect_phase(args.collect)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "digests.txt"), "w") as f:
        for k in a:
            f.write("  ".join([a[k], b.get(k, "-"), k]) + "\n")
        f.write("# columns: " + "  ".join(args.libs) + "  case\n")
    with open(os.path.join(args.out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0 if res["digests_equal"] else 1)


if __name__ == "__main__":
    main()

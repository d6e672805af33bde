#!/usr/bin/env python3
"""A/B of one deployment step of the image-conditioned DPT (what MiniworldTransformerController.act costs
per env step), three arms in one process.

Arm "session": ``dpt_hip.ImageActSession.act`` on raw uint8 60 x 80 host frames -- the frame upload, the
fused front kernel (resize, normalise, encode and embed the query frame), the trunk on the window, the
action choice and the read-back of the actions.  The context rows were encoded once (``set_context``).
Arm "module": the means of the code before the act step: frames already resized, normalised and on the
device, then ``model(batch)`` on the whole window (all 1 + C images through the encoder), the same action
choice and read-back.  It isolates the encoder and trunk saving.
Arm "module_host_pre": the same plus the host preprocessing a user of that code had to write: the
scipy.ndimage restatement of skimage's anti-aliased resize per frame, the normalisation and the upload.

Shapes: the reference's online (B = 20) and offline (B = 100) evaluations at C = 50 context rows, width
32, four layers.  The arms warm up, then alternate over ``--rounds`` rounds; every round starts and ends
in a device synchronise and is timed with the host clock.  The spread of an arm is (max - min) / median
of its round times; a difference between two arms counts only where it exceeds the spread of both.

Writes one JSON document (default profiles/image_act/ab.json).  Needs the GPU: there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SD, A = 2, 4
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


def host_preprocess(frames):
    """(B, h, w, 3) uint8 -> (B, 3, 25, 25) float32: skimage's resize(..., anti_aliasing=True) restated on
    scipy.ndimage, then ToTensor + Normalize, frame by frame as the reference's controller does"""
    from scipy import ndimage
    out = []
    for f in frames:
        x = f.astype(np.float64) / 255
        sig = np.maximum(0, (np.array(x.shape[:2]) / 25 - 1) / 2)
        x = ndimage.gaussian_filter(x, (sig[0], sig[1], 0), mode="mirror", truncate=4.0)
        x = ndimage.zoom(x, (25 / x.shape[0], 25 / x.shape[1], 1), order=1, mode="mirror", grid_mode=True)
        out.append(((x - MEAN) / STD).transpose(2, 0, 1))
    return np.stack(out).astype(np.float32)


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_step_rounds": [round(x, 3) for x in per_step], "ms_per_step_median": round(med, 3),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_steps": steps * len(times)}


def compare(res, slow, fast):
    """ratio fast / slow of the medians, and whether the difference exceeds both arms' spreads"""
    s, f = res[slow]["ms_per_step_median"], res[fast]["ms_per_step_median"]
    gap = abs(s - f) / min(s, f)
    exceeds = bool(gap > res[slow]["spread"] and gap > res[fast]["spread"])
    return {"ratio": round(f / s, 4), "difference_exceeds_both_spreads": exceeds,
            f"{fast}_is_faster": bool(f < s and exceeds)}


def measure(model, B, C, hw, args):
    import dpt_hip
    dev = dpt_hip.device()
    rs = np.random.RandomState(B)
    ctx = {"context_images": torch.as_tensor(rs.normal(size=(B, C, 3, 25, 25)), dtype=torch.float32, device=dev),
           "context_states": torch.as_tensor(rs.normal(size=(B, C, SD)), dtype=torch.float32, device=dev),
           "context_actions": torch.as_tensor(np.eye(A)[rs.randint(0, A, (B, C))], dtype=torch.float32, device=dev),
           "context_rewards": torch.as_tensor(rs.uniform(size=(B, C, 1)), dtype=torch.float32, device=dev)}
    # a few distinct host frame batches, cycled: every step uploads one
    frames = [rs.randint(0, 256, (B, *hw, 3)).astype(np.uint8) for _ in range(8)]
    angles = [rs.normal(size=(B, SD)).astype(np.float32) for _ in range(8)]
    session = dpt_hip.ImageActSession(model, B, hw)
    session.set_context(ctx)
    obs_dev = [dpt_hip.obs_preprocess(f).clone() for f in frames]
    angle_dev = [torch.as_tensor(a, device=dev) for a in angles]
    counter = [0]

    def arm_session(k):
        for i in range(k):
            counter[0] += 1
            session.act(frames[i % 8], angles[i % 8], True, seed=1, counter=counter[0]).cpu()
        return k

    def module_step(obs, angle):
        counter[0] += 1
        logits = model(dict(ctx, query_images=obs, query_states=angle))
        dpt_hip.select_action(logits, True, 1.0, seed=1, counter=counter[0]).cpu()

    def arm_module(k):
        for i in range(k):
            module_step(obs_dev[i % 8], angle_dev[i % 8])
        return k

    def arm_module_host_pre(k):
        for i in range(k):
            obs = torch.as_tensor(host_preprocess(frames[i % 8])).to(dev)
            module_step(obs, torch.as_tensor(angles[i % 8]).to(dev))
        return k

    # the arms compute the same step: compare the logits once before timing
    session.act(frames[0], angles[0], False)
    with torch.no_grad():
        plain = model(dict(ctx, query_images=obs_dev[0], query_states=angle_dev[0]))
    agree = float((session.logits - plain).abs().max())

    arms = {"session": (arm_session, args.steps), "module": (arm_module, args.steps),
            "module_host_pre": (arm_module_host_pre, args.host_steps)}
    arms = {a: v for a, v in arms.items() if a in args.arms}
    with torch.no_grad():
        for a, (fn, k) in arms.items():
            fn(2 if a == "module_host_pre" else args.warmup)
        torch.cuda.synchronize()
        times, steps = {a: [] for a in arms}, {}
        for _ in range(args.rounds):
            for a, (fn, k) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps[a] = fn(k)
                torch.cuda.synchronize()
                times[a].append(time.perf_counter() - t0)
    res = {"batch": B, "context": C, "window": C + 1, "frame": list(hw),
           "images_encoded_per_step": {"session": B, "module": B * (C + 1)},
           "max_logit_difference_session_vs_module": agree}
    res.update({a: summary(t, steps[a]) for a, t in times.items()})
    if "session" in arms and "module" in arms:
        res["session_over_module"] = compare(res, "module", "session")
    if "session" in arms and "module_host_pre" in arms:
        res["session_over_module_host_pre"] = compare(res, "module_host_pre", "session")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000,
                    help="steps per timed round of the two device arms (a round of about a second)")
    ap.add_argument("--host-steps", type=int, default=100, help="steps per timed round of the host-preprocessing arm")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=200, help="untimed steps per device arm first")
    ap.add_argument("--arms", nargs="+", default=["session", "module", "module_host_pre"],
                    help="the arms to run (one arm alone for a kernel trace)")
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_act", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_act_ab.py measures on the GPU; none is visible")
    import dpt_hip
    from models.net import ImageTransformer
    dev = dpt_hip.device()
    torch.manual_seed(0)
    model = ImageTransformer(dict(horizon=args.H, state_dim=SD, action_dim=A, n_layer=args.layer, n_embd=args.embd,
                                  n_head=4, dropout=0.0, test=True, image_size=25)).to(dev).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    res = {"device": torch.cuda.get_device_name(0), "n_embd": args.embd, "n_layer": args.layer, "state_dim": SD,
           "action_dim": A, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "arms": {"session": "ImageActSession.act on host uint8 frames: upload, fused front kernel, trunk, "
                               "dpt_select_action, actions read back",
                    "module": "frames already normalised on the device, model(batch) on the whole window, "
                              "dpt_select_action, actions read back",
                    "module_host_pre": "module plus the scipy.ndimage resize and normalisation on the host and the "
                                       "upload of the result"},
           "shapes": [measure(model, B, args.H, (60, 80), args) for B in args.batches]}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

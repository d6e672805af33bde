#!/usr/bin/env python3
"""A/B of one ImageTransformer training step (forward + summed cross-entropy + backward, no optimizer)
at the reference's miniworld shape, in one process.

Arm "torch_front": the image front end as plain torch modules on the device under autograd
(``nn.Conv2d`` / ``nn.Linear`` / ``nn.LayerNorm``, the library kernels torch picks) feeding the trunk's
training kernels through dpt_train_forward_embeds / dpt_train_backward_embeds -- what the trunk kernels
plus torch could do without the HIP front end.  Arm "fused_front": ``ImageTransformerFunction`` (the HIP
front end chained into the same trunk kernels).  Both arms pack their parameters every step, as a
training step does.  "front_only" rounds time each arm's front end alone (forward + backward from a
fixed dL/dembeds); the front end's share of the step is that time over the step's.

Shape: batch 64, window 51 (3,264 images a step), width 32, four layers, state_dim 2, action_dim 4.
Both arms warm up, then run ``--rounds`` alternating rounds of ``--steps`` steps; every round starts and
ends in a device synchronise and is timed with the host clock.  The spread of an arm is
(max - min) / median of its round times; the fused arm counts as faster only where the difference
between the medians exceeds the spread of both arms.

Writes one JSON document (default profiles/image_front/ab.json).  Needs the GPU: there is no CPU
fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))

import torch  # noqa: E402


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_step_rounds": [round(x, 3) for x in per_step], "ms_per_step_median": round(med, 3),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_steps": steps * len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed round (a round of about 0.3 s)")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=300,
                    help="untimed steps per arm first (with 3 the first timed rounds were up to 40 %% slower)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_front", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_front_ab.py measures on the GPU; none is visible")
    import dpt_hip
    from dpt_hip import train as tr
    from models.net import ImageTransformer
    dev = dpt_hip.device()
    B, T, E, L, sd, A = args.batch, args.H + 1, args.embd, args.layer, 2, 4
    torch.manual_seed(0)
    model = ImageTransformer(dict(horizon=args.H, state_dim=sd, action_dim=A, n_layer=L, n_embd=E, n_head=4,
                                  shuffle=True, dropout=0.0, test=False, image_size=25)).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(1)
    images = torch.randn(B, T, 3, 25, 25, generator=gen).to(dev)
    feats = torch.randn(B, T, sd + A + 1, generator=gen).to(dev)
    target = torch.eye(A)[torch.randint(0, A, (B,), generator=gen)].to(dev)
    dembeds = torch.randn(B * T, E, generator=gen).to(dev)
    true = target[:, None, :].expand(B, T - 1, A).reshape(-1, A)
    loss_fn = torch.nn.CrossEntropyLoss(reduction="sum")
    dims = (L, E, sd, A, model.n_positions, B, T, 0, 0.0, 0)
    params = tr.image_param_list(model)
    trunk = params[tr.N_FRONT:]
    emb_numel = (2 * sd + A + 1) * E + E
    d = tr.desc(L, E, sd, A, model.n_positions, B, T)

    class TrunkOnEmbeds(torch.autograd.Function):
        """the trunk's training kernels on caller-made embeddings, differentiable in them and the trunk"""

        @staticmethod
        def forward(ctx, embeds, *ps):
            with torch.no_grad():
                q = [p.detach() for p in ps]
                q[-2] = q[-2].t()
                blob = torch.cat([torch.zeros(emb_numel, device=dev)] + [p.reshape(-1) for p in q])
            preds, ws = tr.forward_embeds(d, blob, embeds.detach().contiguous())
            ctx.keep = (blob, ws, [tuple(p.shape) for p in ps])
            return preds

        @staticmethod
        def backward(ctx, dpreds):
            blob, ws, shapes = ctx.keep
            dblob, de = tr.backward_embeds(d, blob, ws, dpreds)
            out, off = [], emb_numel
            for i, sh in enumerate(shapes):
                n = int(torch.Size(sh).numel())
                flat = dblob[off:off + n]
                out.append(flat.view(sh[1], sh[0]).t() if i == len(shapes) - 2 else flat.view(sh))
                off += n
            return (de,) + tuple(out)

    def torch_front():
        x = model.image_encoder(images.view(B * T, 3, 25, 25))
        return model.embed_ln(model.embed_transition(torch.cat([x, feats.view(B * T, -1)], dim=1)))

    def step_torch(k):
        for _ in range(k):
            model.zero_grad(set_to_none=True)
            preds = TrunkOnEmbeds.apply(torch_front().view(B, T, E), *trunk)
            loss_fn(preds[:, 1:].reshape(-1, A), true).backward()

    def step_fused(k):
        for _ in range(k):
            model.zero_grad(set_to_none=True)
            preds = tr.ImageTransformerFunction.apply(images, feats, dims, *params)
            loss_fn(preds[:, 1:].reshape(-1, A), true).backward()

    def front_torch(k):
        for _ in range(k):
            model.zero_grad(set_to_none=True)
            torch_front().backward(dembeds)

    fd = tr.image_desc(B * T, sd, A, E)
    img2, ft2 = images.view(B * T, 3, 25, 25), feats.view(B * T, -1)

    def front_fused(k):
        for _ in range(k):
            fblob, _ = tr.pack_image_params(params, emb_numel, dev)
            embeds, ws = tr.front_forward(fd, fblob, img2, ft2)
            tr.front_backward(fd, fblob, img2, ft2, ws, dembeds)

    # both arms compute the same step: compare the gradients once before timing
    step_torch(1)
    g_torch = [p.grad.clone() for p in params]
    step_fused(1)
    agree = max(float((p.grad - g).abs().max() / g.abs().max()) for p, g in zip(params, g_torch))

    arms = {"torch_front": step_torch, "fused_front": step_fused, "torch_front_only": front_torch,
            "fused_front_only": front_fused}
    times = {a: [] for a in arms}
    for fn in arms.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.steps)
            torch.cuda.synchronize()
            times[a].append(time.perf_counter() - t0)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "window": T, "images_per_step": B * T, "n_embd": E,
           "n_layer": L, "state_dim": sd, "action_dim": A, "rounds": args.rounds, "steps_per_round": args.steps,
           "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "step": "forward + summed cross-entropy + backward, parameters packed every step, no optimizer",
           "arms_gradient_disagreement_of_max": agree}
    res.update({a: summary(t, args.steps) for a, t in times.items()})
    t_med, f_med = res["torch_front"]["ms_per_step_median"], res["fused_front"]["ms_per_step_median"]
    res["fused_over_torch"] = round(f_med / t_med, 4)
    gap = abs(t_med - f_med) / min(t_med, f_med)
    res["difference_exceeds_both_spreads"] = bool(gap > res["torch_front"]["spread"] and
                                                  gap > res["fused_front"]["spread"])
    res["fused_is_faster"] = bool(f_med < t_med and res["difference_exceeds_both_spreads"])
    res["front_share_of_step"] = {
        "torch_front": round(res["torch_front_only"]["ms_per_step_median"] / t_med, 4),
        "fused_front": round(res["fused_front_only"]["ms_per_step_median"] / f_med, 4)}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""A/B of library builds (Makefile `variant`): one bandit rollout timing per library,
each in its own process (python scripts/ab_lib.py libA.so libB.so ...; rounds alternate).
An argument libX.so:<bytes> runs libX.so with dpt_hip.set_cache_budget(<bytes>); the suffixes +nows / +nomemo
run DarkRoom without the layer-0 workspace / the logits memo (in that order: lib.so+nows+nomemo); a last suffix
+y32 / +y24 sets dpt_hip.set_ycache_bits (a build without that key fails when it is set).  libX.so@<file>.py
(before any other suffix) loads that file in place of dpt_hip/train.py: an A/B of the Python layer on one library.
Env: AB_H, AB_N, AB_A, AB_TILE, AB_ROUNDS.
AB_WL=train: the training entry points instead (trunk forward / backward, generic rollout, the three
cross-entropies, the fused steps and the four trainer classes over several steps, the trunk's and the generic
rollout's workspace sizes): one sha1 per case over
the raw bytes of every output (group 5: the width-32 window forward, the DarkRoom episode rollout, the
interactive DarkRoom step and the chains' workspace sizes), then the ms per dpt_train_step at the shapes of
scripts/train_timing.py (AB_STEPS steps between device events), the host microseconds to enqueue one step of each
trainer, and the ms per call of the window forward, the episode rollout and the interactive DarkRoom step
(``window_ms``).  AB_DIGEST_ROUNDS: compute the digests in that many first rounds only.
The parent exits 1 when two arguments' digests differ and writes digests.txt / ab.json to AB_OUT
(default profiles/train_refactor); ab.json's ``over_margin`` lists the figures whose median exceeds the
first argument's by more than the first argument's own max - min."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def train_digests():
    """{case: sha1} of every output the training entry points write, each case seeded."""
    import torch
    from types import SimpleNamespace
    from dpt_hip import _lib, _p, _stream
    import dpt_hip.train as tr
    from models.net import Transformer
    out = {}
    dev = torch.device("cuda")

    def rnd(rs, *shape, scale=1.0):
        return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).to(dev)

    # 1. the trunk, through the token and the embeds entry
    sd, A, L, B = 1, 5, 2, 3
    FO, LO, LL = tr.FORWARD_ONLY, tr.LAST_ONLY, tr.LAST_LOSS
    for E in (16, 18, 32, 48, 64):
        for T in (1, 2, 65):
            for flags, p in ((0, 0.0), (FO, 0.0), (FO | LO, 0.0), (LL, 0.0), (0, 0.1), (FO, 0.1)):
                rs = np.random.RandomState(1000 * E + 10 * T + flags)
                d = tr.desc(L, E, sd, A, 72, B, T, flags=flags, dropout=p, seed=4242)
                blob = rnd(rs, tr._numel("dpt_train_blob_numel", d), scale=0.1)
                dp = rnd(rs, B, T, A)
                if flags & LL:
                    dp[:, :-1] = 0
                for entry, x in (("tokens", rnd(rs, B, T, 2 * sd + A + 1)), ("embeds", rnd(rs, B, T, E))):
                    preds, ws = (tr.forward if entry == "tokens" else tr.forward_embeds)(d, blob, x)
                    outs = [preds[:, -1] if flags & (LO | LL) else preds]  # the last-position modes write that row alone
                    if not flags & FO:
                        outs += [tr.backward(d, blob, x, ws, dp)] if entry == "tokens" else \
                            list(tr.backward_embeds(d, blob, ws, dp))
                    out[f"trunk E{E} T{T} flags{flags} drop{p} {entry}"] = sha(*outs)
    # 2. the generic rollout past one 64-key lap
    N, H = 9, 70
    for E in (16, 18, 20, 32, 48, 64, 128, 256):
        for name, code in (("gaussian", _lib.BANDIT_GAUSSIAN), ("bernoulli", _lib.BANDIT_BERNOULLI)):
            rs = np.random.RandomState(7 * E + code)
            shape = SimpleNamespace(n_layer=L, n_embd=E, state_dim=1, action_dim=A, n_positions=72)
            blob = rnd(rs, tr._numel("dpt_train_blob_numel", tr.desc(L, E, 1, A, 72, 1, 1)), scale=0.1)
            o = tr.rollout_bandit_generic(shape, rs.uniform(0, 1, (N, A)), H, 0.3, True, code, seed=11,
                                          want_logits=True, blob=blob)
            out[f"rollout E{E} {name}"] = sha(o["actions"], o["rewards"], o["logits"])
    # the trunk's and the rollout's workspace sizes, training and forward-only
    for E in (16, 18, 20, 32, 128):
        sizes = []
        for flags in (0, FO):
            for B_, T_ in ((1, 1), (3, 65), (64, 501)):
                sizes.append(tr._numel("dpt_train_workspace_numel", tr.desc(L, E, sd, A, 2004, B_, T_, flags=flags)))
            for N_, H_ in ((1, 1), (9, 70), (1000, 500)):
                need = ctypes.c_int64(-1)
                _lib.call("dpt_rollout_bandit_generic_workspace_numel",
                          ctypes.byref(tr.desc(L, E, sd, A, 2004, 1, 1, flags=flags)), N_, H_, ctypes.byref(need))
                sizes.append(need.value)
        out[f"workspace sizes E{E}"] = sha(torch.tensor(sizes, dtype=torch.int64))
    # 3. the loss kernels: one target out of range, one weight 0
    for B_, T_, A_ in ((3, 1, 5), (4, 9, 20), (2, 5, 1)):
        rs = np.random.RandomState(100 * B_ + A_)
        preds = rnd(rs, B_, T_, A_, scale=3.0)
        soft = torch.eye(A_, device=dev)[torch.from_numpy(rs.randint(0, A_, B_)).to(dev)].contiguous()
        tseq = torch.from_numpy(rs.randint(0, A_, B_)).to(dev)
        tseq[0] = A_
        trow = torch.from_numpy(rs.randint(0, A_, (B_, T_)).astype(np.int32)).to(dev)
        trow[-1, -1] = -1
        w = torch.from_numpy(rs.uniform(0.5, 2.0, (B_, T_))).to(dev)
        w[0, 0] = 0.0
        sc = ctypes.c_double(1.0 / B_)

        def bufs(rows):
            return (torch.zeros_like(preds), torch.zeros(rows, dtype=torch.float64, device=dev),
                    torch.full((1,), 0.5, dtype=torch.float64, device=dev))

        dpr, part, acc = bufs(B_)
        _lib.call("dpt_train_ce_loss", _p(preds), _p(soft), B_, T_, A_, _p(dpr), _p(part), _p(acc), _stream())
        out[f"ce_loss {B_} {T_} {A_}"] = sha(dpr, part, acc)
        dpr, part, acc = bufs(B_)
        _lib.call("dpt_train_ce_last", _p(preds), _p(tseq), B_, T_, A_, sc, _p(dpr), _p(part), _p(acc), _stream())
        out[f"ce_last {B_} {T_} {A_}"] = sha(dpr, part, acc)
        for form, ts, tw, ww in (("seq", tseq, None, None), ("row weighted", None, trow, w)):
            dpr, part, acc = bufs(B_ * T_)
            _lib.call("dpt_train_ce_rows", _p(preds), _p(ts), _p(tw), _p(ww), B_, T_, A_, sc, _p(part), _p(dpr),
                      _p(acc), _stream())
            out[f"ce_rows {form} {B_} {T_} {A_}"] = sha(dpr, part, acc)
    # 4. the fused steps (the blobs after AdamW, the gradient blobs, the losses)
    for E in (32, 18):
        def model(seed, H_, dropout=0.0):
            torch.manual_seed(seed)
            return Transformer(dict(horizon=H_, state_dim=1, action_dim=A, n_layer=L, n_embd=E, n_head=1,
                                    dropout=dropout, test=False)).cuda().train()

        rs = np.random.RandomState(E)
        t = tr.Trainer(model(1, 8), lr=1e-3)
        t.step(step_data(rs, 12, 8, 1, A), np.arange(2, 8))
        out[f"train_step E{E}"] = sha(t.blob, t.m, t.v, t.loss)
        means = rs.uniform(0, 1, (8, A))
        for chunk in (0, 3):  # 3: the later chunks accumulate
            t = tr.InteractiveTrainer(model(2, 8), lr=1e-3, chunk=chunk)
            acts, rew = t.step(means, 6, 0.3, "uniform", seed=5)
            out[f"interactive E{E} chunk{chunk}"] = sha(t.blob, t.dblob, t.loss, acts, rew)
        t = tr.ExploreExploitTrainer(model(3, 8), model(4, 8), lr=1e-3)
        recs = t.step(means, 6, 0.3, "bernoulli", 0.5, seed=6)
        out[f"explore E{E}"] = sha(t.explorer_blob, t.exploiter_blob, t.explorer_dblob, t.exploiter_dblob,
                                   t.loss_explorer, t.loss_exploiter, *recs)
        trainer_digests(out, tr, model, E, A, L)
    window_digests(out, tr)
    return out


def window_digests(out, tr):
    """Group 5: the width-32 window forward (prefill) and what is built on it or beside it -- the one-launch
    DarkRoom episode rollout, the interactive DarkRoom step and its two kernels called directly, and the three
    chains' workspace sizes.  Two layers, three sequences / envs, at the smallest windows that reach every
    geometry (4, 8 and 16 waves) and both parities of the 16-token block count."""
    import torch
    import dpt_hip
    from dpt_hip import _lib, _p, _stream
    from models.net import Transformer
    dev, A, L = torch.device("cuda"), 5, 2

    def model(seed, H, sd, E=32):
        torch.manual_seed(seed)
        return Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=L, n_embd=E, n_head=1, dropout=0.0,
                                test=False)).cuda().train()

    # dpt_forward_window on the prefill
    for env, sd in (("bandit", 1), ("darkroom", 2)):
        dm = model(40 + sd, 256, sd).device_model()
        for T in (1, 16, 17, 33, 128, 129, 257):
            rs, C = np.random.RandomState(100 * sd + T), T - 1
            data = step_data(rs, 3, C, sd, A)
            ctx = [data[k].to(dev) for k in ("context_states", "context_actions", "context_next_states",
                                             "context_rewards")] if C else [None] * 4
            for mode in (0, 1):
                out[f"forward_window {env} T{T} out_mode{mode}"] = sha(
                    dm.forward_window(data["query_states"].to(dev), *ctx, out_mode=mode))
    # dpt_rollout_darkroom_episode
    dim = 5
    for K in (2, 17, 33, 129, 257):
        m = model(50, 256, 2).eval()
        rs = np.random.RandomState(K)
        goals = rs.randint(0, dim, (3, 2)).astype(np.int32)
        perm = np.stack([rs.permutation(A) for _ in range(3)]).astype(np.int32)
        u = rs.uniform(0, 1, (K - 1, 3))
        for name, kw in (("greedy", dict(sample=False)), ("sampled seed", dict(sample=True, seed=9)),
                         ("sampled uniforms", dict(sample=True, uniforms=u))):
            for pm in (None, perm):
                rec, ret, lg = dpt_hip.rollout_darkroom_episode(m, goals, K, dim, perm=pm, logits=True, **kw)
                out[f"episode K{K} {name} perm{int(pm is not None)}"] = sha(
                    rec["states"], rec["actions"], rec["rewards"], rec["targets"], lg, ret)
    # dpt_interactive_mdp_grad through InteractiveMDPTrainer: 5 envs, K = 4
    K, rs = 4, np.random.RandomState(60)
    goals = rs.randint(0, dim, (5, 2)).astype(np.int32)
    for E in (32, 18):
        for chunk in (0, 2):  # 2: the later chunks accumulate
            for loss in ("every", "last"):
                t = tr.InteractiveMDPTrainer(model(61, 8, 2, E), lr=1e-3, chunk=chunk, loss=loss)
                rec = t.step(goals, K, dim, seed=13)
                out[f"InteractiveMDPTrainer E{E} chunk{chunk} loss {loss}"] = sha(
                    t.blob, t.m, t.v, t.dblob, t.loss, *(rec[k] for k in sorted(rec)))
            rec, ret = t.rollout(goals, K, dim, sample=True, seed=14)
            out[f"InteractiveMDPTrainer E{E} chunk{chunk} rollout"] = sha(ret, *(rec[k] for k in sorted(rec)))
    # dpt_mdp_pack and dpt_darkroom_act_step called directly: N = 3, K = 4, t = 0 and 2
    N = 3
    for t in (0, 2):
        rs = np.random.RandomState(70 + t)
        i32 = lambda v: torch.from_numpy(np.asarray(v).astype(np.int32)).to(dev)  # noqa: E731
        states, actions = i32(rs.randint(0, dim, (N, K, 2))), i32(rs.randint(0, A, (N, K - 1)))
        rewards, targets = i32(rs.randint(0, 2, (N, K - 1))), i32(rs.randint(0, A, (N, K)))
        goal, perm = i32(rs.randint(0, dim, (N, 2))), i32(np.stack([rs.permutation(A) for _ in range(N)]))
        tokens = torch.zeros((N, t + 1, 10), dtype=torch.float32, device=dev)
        _lib.call("dpt_mdp_pack", _p(states), _p(actions), _p(rewards), N, K, t, _p(tokens), _stream())
        out[f"mdp_pack t{t}"] = sha(tokens)
        logits = torch.from_numpy(rs.standard_normal((N, t + 1, A)).astype(np.float32)).to(dev)
        for sample, pm in ((0, None), (1, None), (1, perm)):
            rec = [x.clone() for x in (states, actions, rewards, targets)]
            nxt = torch.zeros(N, dtype=torch.int64, device=dev)
            _lib.call("dpt_darkroom_act_step", _p(logits), N, t + 1, K, t, dim, sample, None, 17, t, 0, _p(goal),
                      _p(pm), *(_p(x) for x in rec), _p(nxt), _stream())
            out[f"darkroom_act_step t{t} sample{sample} perm{int(pm is not None)}"] = sha(*rec, nxt)
    # the chains' workspace sizes (a rejected shape digests as -1)
    for sd, fns in ((1, (("dpt_interactive_workspace_numel", ()), ("dpt_explore_workspace_numel", ()))),
                    (2, tuple(("dpt_interactive_mdp_workspace_numel", (mode,)) for mode in sorted(tr.MDP_LOSS.values())))):
        d = tr.desc(L, 32, sd, A, 36, 1, 1)
        for fn, extra in fns:
            sizes, said = [], ""
            for K in (1, 2, 6):
                for N in (1, 8):
                    need = ctypes.c_int64(-1)
                    try:
                        _lib.call(fn, ctypes.byref(d), N, K, *extra, ctypes.byref(need))
                    except ValueError as e:  # the explorer's K = 1: its message goes into the digest
                        said += str(e)
                    sizes.append(need.value)
            out[f"{fn} {extra} K 1,2,6 x N 1,8"] = sha(torch.tensor(sizes, dtype=torch.int64),
                                                         torch.tensor(list(said.encode()), dtype=torch.uint8))


def image_arrays(rs, n, H, sd, A):
    """a collated batch dict for DeviceImageData.from_arrays (the images count as normalised already)"""
    import torch
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    return {"query_states": f32(rs.normal(size=(n, sd))), "context_states": f32(rs.normal(size=(n, H, sd))),
            "context_actions": f32(np.eye(A)[rs.randint(0, A, (n, H))]),
            "context_rewards": f32(rs.normal(size=(n, H))), "optimal_actions": f32(np.eye(A)[rs.randint(0, A, n)]),
            "query_images": f32(rs.normal(size=(n, 3, 25, 25))),
            "context_images": f32(rs.normal(size=(n, H, 3, 25, 25)))}


def trainer_digests(out, tr, model, E, A, L):
    """Group 4 continued: the four trainer classes through their public surface alone -- three steps (the
    second on a smaller batch), ``eval_loss``, dropout seeds from the CUDA generator and passed in, chunked
    gradients, and the state after a rejected call.  ``model(seed, H, dropout)``: a Transformer."""
    import torch
    from models.net import ImageTransformer

    def weights(*modules):
        return [q for m in modules for _, q in sorted(m.state_dict().items())]

    def rejected(name, t, blob, call):
        """a call the trainer must refuse, then (by the caller) a good one: steps and blob stay"""
        steps, before = t.steps, blob.clone()
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError(f"{name}: the call was not rejected")
        out[name] = sha(blob, torch.tensor([t.steps, steps, int(torch.equal(blob, before))]))

    # Trainer: batches of 6, 4 (with a perm) and 6 samples, then the test loss; dropout seeds are drawn per call
    H = 8
    for p in (0.0, 0.1):
        rs = np.random.RandomState(100 + E)
        data = step_data(rs, 12, H, 1, A)
        perm = np.stack([rs.permutation(H) for _ in range(4)])
        t = tr.Trainer(model(5, H, p), lr=1e-3)
        torch.cuda.manual_seed(1)
        t.step(data, np.arange(0, 6))
        t.step(data, np.arange(6, 10), perm=perm)
        t.step(data, np.arange(3, 9))
        t.eval_loss(data, np.arange(1, 6))
        out[f"Trainer E{E} drop{p} steps 6,4p,6 + eval"] = sha(t.blob, t.m, t.v, t.loss, torch.tensor([t.steps]))
        if p == 0.0:
            rejected(f"Trainer E{E} rejects action_dim", t, t.blob,
                     lambda: t.step(step_data(rs, 4, H, 1, A + 1), np.arange(4)))
            rejected(f"Trainer E{E} rejects a window above n_positions", t, t.blob,
                     lambda: t.step(step_data(rs, 4, 5 * H, 1, A), np.arange(4)))
            rejected(f"Trainer E{E} rejects perm", t, t.blob, lambda: t.eval_loss(data, np.arange(4), perm=perm[:3]))
            t.step(data, np.arange(2, 7))
            out[f"Trainer E{E} step after the rejected ones"] = sha(t.blob, t.m, t.v, t.loss, torch.tensor([t.steps]))
    # ImageTrainer on 6 synthetic samples of horizon 3
    sd, Hi = 2, 3
    for p, seeds, name in ((0.0, None, "drop0.0"), (0.1, (11, 12, 13, 14), "drop0.1 seed="),
                           (0.1, None, "drop0.1 seed=None")):
        rs = np.random.RandomState(200 + E)
        data = tr.DeviceImageData.from_arrays(image_arrays(rs, 6, Hi, sd, A))
        perm = np.stack([rs.permutation(Hi) for _ in range(2)])
        torch.manual_seed(6)
        t = tr.ImageTrainer(ImageTransformer(dict(
            horizon=Hi, state_dim=sd, action_dim=A, n_layer=L, n_embd=E, n_head=1, shuffle=False, dropout=p, test=False,
            store_gpu=False, image_size=25)).cuda().train(), lr=1e-3)
        torch.cuda.manual_seed(1)
        s = seeds or (None,) * 4
        t.step(data, np.arange(0, 4), seed=s[0])
        t.step(data, np.arange(4, 6), perm=perm, seed=s[1])
        t.step(data, np.arange(1, 5), seed=s[2])
        t.eval_loss(data, np.arange(0, 3), seed=s[3])
        state = (t.blob, t.front_blob, t.m, t.v, t.front_m, t.front_v, t.loss)
        out[f"ImageTrainer E{E} {name} steps 4,2p,4 + eval"] = sha(*state, torch.tensor([t.steps]))
        if p == 0.0:
            rejected(f"ImageTrainer E{E} rejects action_dim", t, t.front_blob,
                     lambda: t.step(tr.DeviceImageData.from_arrays(image_arrays(rs, 2, Hi, sd, A + 1)), np.arange(2)))
            t.step(data, np.arange(2, 5))
            out[f"ImageTrainer E{E} step after the rejected one"] = sha(*state, torch.tensor([t.steps]))
            out[f"ImageTrainer E{E} sync_to_model"] = sha(*weights(t.sync_to_model()))
    # the bandit pair: 8 envs, then 5 (another workspace), then 8; K = 6 (window 6 of n_positions 36)
    K = 6
    rs = np.random.RandomState(300 + E)
    means = rs.uniform(0, 1, (8, A))
    u5, g5 = rs.uniform(0, 1, (K - 1, 5)), rs.standard_normal((K - 1, 5))
    ea8 = rs.randint(0, A, (K - 1, 8)).astype(np.int32)
    for chunk in (0, 3):
        for fw in (False, True):
            t = tr.InteractiveTrainer(model(7, 8), lr=1e-3, chunk=chunk, full_width=fw)
            recs = list(t.step(means, K, 0.3, "uniform", seed=21))
            recs += t.step(means[:5], K, 0.3, "bernoulli", uniforms=u5, noise=g5, targets=np.arange(5) % A)
            recs += t.step(means, K, 0.3, "uniform", seed=22)
            out[f"InteractiveTrainer E{E} chunk{chunk} full_width{int(fw)} envs 8,5,8"] = sha(
                t.blob, t.m, t.v, t.dblob, t.loss, torch.tensor([t.steps]), *recs)
        rejected(f"InteractiveTrainer E{E} chunk{chunk} rejects uniforms", t, t.blob,
                 lambda: t.step(means, K, 0.3, "uniform", uniforms=u5))
        rejected(f"InteractiveTrainer E{E} chunk{chunk} rejects K above n_positions", t, t.blob,
                 lambda: t.step(means, 37, 0.3, "uniform", seed=1))
        t.step(means, K, 0.3, "uniform", seed=23)
        out[f"InteractiveTrainer E{E} chunk{chunk} step after the rejected ones"] = sha(
            t.blob, t.m, t.v, t.dblob, t.loss, torch.tensor([t.steps]))
        out[f"InteractiveTrainer E{E} chunk{chunk} sync_to_model"] = sha(*weights(t.sync_to_model()))
        for inject in (False, True):
            t = tr.ExploreExploitTrainer(model(8, 8), model(9, 8), lr=1e-3, chunk=chunk)
            recs = list(t.step(means, K, 0.3, "bernoulli", 0.5, seed=31, env_actions=ea8 if inject else None))
            recs += t.step(means[:5], K, 0.3, "uniform", 0.5, uniforms=u5, noise=g5)
            recs += t.step(means, K, 0.3, "bernoulli", 2.0, seed=32)
            blobs = (t.explorer_blob, t.exploiter_blob, t.explorer_dblob, t.exploiter_dblob)
            out[f"ExploreExploitTrainer E{E} chunk{chunk} env_actions{int(inject)} envs 8,5,8"] = sha(
                *blobs, t.loss_explorer, t.loss_exploiter, torch.tensor([t.steps]), *recs)
        rejected(f"ExploreExploitTrainer E{E} chunk{chunk} rejects env_actions", t, t.explorer_blob,
                 lambda: t.step(means, K, 0.3, "uniform", 1.0, env_actions=ea8[:, :5]))
        rejected(f"ExploreExploitTrainer E{E} chunk{chunk} rejects beta", t, t.exploiter_blob,
                 lambda: t.step(means, K, 0.3, "uniform", 0.0, seed=1))
        t.step(means, K, 0.3, "uniform", 1.0, seed=33)
        losses = t.read_losses()
        out[f"ExploreExploitTrainer E{E} chunk{chunk} step after the rejected ones"] = sha(
            *blobs, torch.tensor(losses, dtype=torch.float64), t.loss_explorer, t.loss_exploiter,
            torch.tensor([t.steps]))
        out[f"ExploreExploitTrainer E{E} chunk{chunk} sync_to_models"] = sha(*weights(*t.sync_to_models()))


def step_data(rs, n, H, sd, A):
    import torch
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    return {"query_states": f32(rs.randint(0, 10, (n, sd))), "context_states": f32(rs.randint(0, 10, (n, H, sd))),
            "context_actions": f32(np.eye(A)[rs.randint(0, A, (n, H))]),
            "context_next_states": f32(rs.randint(0, 10, (n, H, sd))),
            "context_rewards": f32(rs.normal(0.5, 0.5, (n, H, 1))),
            "optimal_actions": f32(np.eye(A)[rs.randint(0, A, n)])}


def train_child(lib):
    """AB_WL=train: the digests, then ms per dpt_train_step (forward, cross-entropy, backward, AdamW) at
    scripts/train_timing.py's shapes -- width 32, 4 layers, batch 64."""
    import torch
    import dpt_hip.train as tr
    from models.net import Transformer
    digests = train_digests() if os.environ.get("AB_DIGEST", "1") == "1" else {}
    steps, ms = int(os.environ.get("AB_STEPS", "300")), {}
    for name, sd, A, H, B in (("bandit_T501", 1, 5, 500, 64), ("darkroom_T101", 2, 5, 100, 64)):
        torch.manual_seed(0)
        rs = np.random.RandomState(0)
        t = tr.Trainer(Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=4, n_embd=32, n_head=1,
                                        dropout=0.0, test=False)).cuda().train(), lr=1e-4)
        dd = t.device_data(step_data(rs, 4 * B, H, sd, A))
        idx = [torch.from_numpy(rs.randint(0, 4 * B, B)).cuda() for _ in range(16)]
        for i in range(20):
            t.step(dd, idx[i % 16])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(steps):
            t.step(dd, idx[i % 16])
        b.record()
        torch.cuda.synchronize()
        ms[name] = a.elapsed_time(b) / steps
    print(json.dumps({"lib": lib, "digests": digests, "ms": ms, "host_us": host_us_per_step(tr),
                      "ms_per_call": window_ms(tr)}))


def window_ms(tr):
    """{case: ms per call between device events} of the width-32 window forward and what runs it or beside it,
    four layers, 1024 sequences / envs: dpt_forward_window at windows 101, 201 and 501 (the prefill's 4-, 8- and
    16-wave geometries), the episode rollout at the shapes of scripts/episode_rollout_ab.py and
    InteractiveMDPTrainer.step at those of scripts/interactive_darkroom_ab.py (dim 10)."""
    import torch
    import dpt_hip
    from envs.gpu_darkroom_env import GPUDarkroomEnv
    from models.net import Transformer
    dev, n, A, dim, out = dpt_hip.device(), 1024, 5, 10, {}

    def model(H):
        torch.manual_seed(H)
        return Transformer(dict(horizon=H, state_dim=2, action_dim=A, n_layer=4, n_embd=32, n_head=1, dropout=0.0,
                                test=True)).to(dev)

    def timed(fn, calls, warmup=2):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    dm = model(500).eval().device_model()
    for T in (101, 201, 501):
        data = step_data(np.random.RandomState(T), n, T - 1, 2, A)
        q, *ctx = (data[k].to(dev) for k in ("query_states", "context_states", "context_actions",
                                             "context_next_states", "context_rewards"))
        out[f"forward_window T{T}"] = timed(lambda: dm.forward_window(q, *ctx), 30)
    for K, mdp_calls in ((25, {"every": 8, "last": 20}), (100, {"every": 3, "last": 8})):
        m = model(K).eval()
        torch.manual_seed(K)
        goals = GPUDarkroomEnv(dim, n, K, dev).goals
        for name, sample in (("greedy", False), ("sampled", True)):
            out[f"episode K{K} {name}"] = timed(
                lambda: dpt_hip.rollout_darkroom_episode(m, goals, K, dim, sample=sample, seed=1), 30)
        for mode, calls in mdp_calls.items():
            t = tr.InteractiveMDPTrainer(model(K), lr=1e-3, weight_decay=1e-4, loss=mode)
            out[f"interactive_mdp K{K} {mode}"] = timed(lambda: t.step(goals, K, dim, seed=1), calls, warmup=1)
    return out


def host_us_per_step(tr, steps=200):
    """{trainer: wall microseconds to enqueue one step}, over ``steps`` steps without a synchronisation, at
    shapes where the Python layer is the cost: width 32, 2 layers, 5 arms, 8 samples / envs, window 9."""
    import time
    import torch
    from models.net import ImageTransformer, Transformer
    A, H, n = 5, 8, 8
    cfg = dict(horizon=H, action_dim=A, n_layer=2, n_embd=32, n_head=1, dropout=0.0, test=False)
    rs = np.random.RandomState(0)
    torch.manual_seed(0)
    bandit = [Transformer(dict(cfg, state_dim=1)).cuda().train() for _ in range(4)]
    image = ImageTransformer(dict(cfg, state_dim=2, shuffle=False, store_gpu=False, image_size=25)).cuda().train()
    means, idx = torch.from_numpy(rs.uniform(0, 1, (n, A))).cuda(), torch.arange(n).cuda()
    t0, t1 = tr.Trainer(bandit[0], lr=1e-4), tr.ImageTrainer(image, lr=1e-4)
    d0 = t0.device_data(step_data(rs, 12, H, 1, A))
    d1 = tr.DeviceImageData.from_arrays(image_arrays(rs, n, H, 2, A))
    t2, t3 = tr.InteractiveTrainer(bandit[1], lr=1e-4), tr.ExploreExploitTrainer(bandit[2], bandit[3], lr=1e-4)
    out = {}
    seeds = iter(range(10 ** 6))
    for name, step in (("Trainer", lambda: t0.step(d0, idx)), ("ImageTrainer", lambda: t1.step(d1, idx)),
                       ("InteractiveTrainer", lambda: t2.step(means, H + 1, 0.3, "uniform", seed=next(seeds))),
                       ("ExploreExploitTrainer", lambda: t3.step(means, H + 1, 0.3, "uniform", 1.0, seed=next(seeds)))):
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(steps):
            step()
        out[name] = (time.perf_counter() - start) / steps * 1e6
        torch.cuda.synchronize()
    return out


def train_parent(libs):
    """Alternating rounds of train_child; one summary line, digests.txt and ab.json under AB_OUT."""
    rounds, dig = {lib: [] for lib in libs}, {}
    same = True
    figures = ("ms_per_step", "host_us_per_step", "ms_per_call")
    digest_rounds = int(os.environ.get("AB_DIGEST_ROUNDS", "1000000"))  # the digests in the first rounds alone
    for rnd in range(int(os.environ.get("AB_ROUNDS", "2"))):
        for lib in libs:
            env = dict(os.environ, AB_DIGEST=os.environ.get("AB_DIGEST", "1") if rnd < digest_rounds else "0")
            cp = subprocess.run([sys.executable, __file__, "--child", lib], capture_output=True, text=True,
                                timeout=300, env=env)
            if cp.returncode:
                sys.exit(f"{lib}: child failed ({cp.returncode})\n{cp.stderr[-3000:]}")
            d = json.loads(cp.stdout.strip().splitlines()[-1])
            rounds[lib].append({"ms_per_step": d["ms"], "host_us_per_step": d["host_us"],
                                "ms_per_call": d["ms_per_call"]})
            print(f"round {rnd} {lib}: {rounds[lib][-1]}", file=sys.stderr, flush=True)
            if rnd < digest_rounds:
                same = same and dig.setdefault(lib, d["digests"]) == d["digests"]  # the same library, run to run
    ref = dig[libs[0]]
    diff = sorted(k for lib in libs for k in set(ref) | set(dig[lib]) if ref.get(k) != dig[lib].get(k))
    res = {"digest_cases": len(ref), "digests_equal": same and not diff, "differing": diff,
           "steps_per_round": int(os.environ.get("AB_STEPS", "300")), **{what: {} for what in figures}}
    for lib, rs_ in rounds.items():
        for what in figures:
            per = {k: [r[what][k] for r in rs_] for k in rs_[0][what]}
            res[what][lib] = {k: {"rounds": [round(x, 5) for x in v], "median": float(np.median(v)), "min": min(v),
                                  "max": max(v)} for k, v in per.items()}
    # every later argument against the first: its median may exceed the first's by the first's own spread
    res["over_margin"] = [
        f"{what} {k} {lib}" for what in figures for lib in libs[1:]
        for k, base in res[what][libs[0]].items()
        if res[what][lib][k]["median"] - base["median"] > base["max"] - base["min"]]
    out = os.environ.get("AB_OUT", os.path.join(ROOT, "profiles", "train_refactor"))
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "digests.txt"), "w") as f:
        for k in ref:
            f.write("  ".join([dig[lib].get(k, "-") for lib in dig] + [k]) + "\n")
        f.write("# columns: " + "  ".join(dig) + "  case\n")
    with open(os.path.join(out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0 if res["digests_equal"] else 1)  # (over_margin is reported, not enforced: read it)


def child(lib):
    sys.path[:0] = [os.path.join(ROOT, "decision-pretrained-transformer_amd"), ROOT]
    from dpt_hip import _lib
    if "@" in lib:  # "libX.so@<file>.py": that file stands in for dpt_hip/train.py (an A/B of the Python layer)
        import importlib.util
        import dpt_hip
        lib, path = lib.split("@", 1)
        spec = importlib.util.spec_from_file_location("dpt_hip.train", os.path.join(ROOT, path))
        dpt_hip.train = sys.modules["dpt_hip.train"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(dpt_hip.train)
    ybits = None  # "libX.so+y32" / "+y24": DPT_TUNE_YCACHE_BITS (the last suffix)
    for suf, bits in (("+y32", 32), ("+y24", 24)):
        if lib.endswith(suf):
            lib, ybits = lib[: -len(suf)], bits
    nomemo = lib.endswith("+nomemo")  # DarkRoom with every step a window forward
    lib = lib[: -len("+nomemo")] if nomemo else lib
    nows = lib.endswith("+nows")  # DarkRoom without the per-episode layer-0 workspace
    lib = lib[: -len("+nows")] if nows else lib
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.__file__), lib.split(":")[0])
    if os.environ.get("AB_WL") == "train":
        return train_child(lib)
    import torch
    import bench
    import dpt_hip
    H, N, A = (int(os.environ.get(k, d)) for k, d in (("AB_H", "500"), ("AB_N", "4096"), ("AB_A", "5")))
    dpt_hip.set_decode_tile(int(os.environ.get("AB_TILE", "8")))
    if ybits is not None:
        dpt_hip.set_ycache_bits(ybits)
    if nomemo:
        dpt_hip.set_darkroom_memo(False)
    if nows:
        dpt_hip.set_darkroom_workspace(False)
    if ":" in lib:  # "libX.so:<bytes>": the same library at another DPT_TUNE_CACHE_BUDGET
        dpt_hip.set_cache_budget(int(lib.split(":")[1]))
    if os.environ.get("AB_WL") == "darkroom":  # config 3: 4096 tasks x 40 episodes x 100 steps
        # AB_DR_R: context episodes (window 1 + 100 R; 1 = config 3)
        R = int(os.environ.get("AB_DR_R", "1"))
        sd, _ = bench.synthetic_state_dict(4, 2, 5, 100 * R)
        m = dpt_hip.DeviceModel(sd, 4, 2, 5, 4 * (1 + 100 * R))
        goals = np.stack(np.unravel_index(np.arange(N) % 100, (10, 10)), 1)
        ts = []
        for rnd in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = m.rollout_darkroom(goals, 40, 100, R, seed=rnd)
            b.record()
            torch.cuda.synchronize()
            if rnd > 0:
                ts.append(a.elapsed_time(b))
        # bit-identity digest: actions and logits of a smaller launch (AB_DIGEST=0 skips it)
        digest = None
        if os.environ.get("AB_DIGEST", "1") == "1":
            import hashlib
            o = m.rollout_darkroom(goals[:512], 6, 100, R, seed=77, want_actions=True, want_logits=True)
            h = hashlib.sha1(o["actions"].cpu().numpy().tobytes())
            h.update(o["logits"].cpu().numpy().tobytes())
            digest = h.hexdigest()[:16]
        print(json.dumps({"lib": lib, "ms": ts, "checksum": float(out["returns"].sum()), "digest": digest}))
        return
    sd, _ = bench.synthetic_state_dict(4, 1, A, H)
    m = dpt_hip.DeviceModel(sd, 4, 1, A, 4 * (1 + H))
    means = torch.from_numpy(np.random.RandomState(1).uniform(0, 1, (N, A))).cuda()
    ts = []
    for rnd in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = m.rollout_bandit(means, H, 0.3, True, seed=rnd)
        b.record()
        torch.cuda.synchronize()
        if rnd > 0:
            ts.append(a.elapsed_time(b))
    chk = float(out["arm_value"].sum())
    print(json.dumps({"lib": lib, "ms": ts, "checksum": chk}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    if os.environ.get("AB_WL") == "train":
        train_parent(sys.argv[1:])  # one library given twice: its own round-to-round spread
    res = {lib: [] for lib in sys.argv[1:]}
    chk = {}
    for rnd in range(int(os.environ.get("AB_ROUNDS", "2"))):
        for lib in sys.argv[1:]:
            cp = subprocess.run([sys.executable, __file__, "--child", lib], capture_output=True, text=True,
                                timeout=300)
            if cp.returncode:
                sys.exit(f"{lib}: child failed ({cp.returncode})\n{cp.stderr[-3000:]}")
            out = cp.stdout.strip().splitlines()[-1]
            d = json.loads(out)
            res[lib] += d["ms"]
            chk[lib] = (d["checksum"], d.get("digest"))
    H, N = int(os.environ.get("AB_H", "500")), int(os.environ.get("AB_N", "4096"))
    sys.path[:0] = [ROOT]
    import bench
    ab = bench.algorithmic_bytes(N, H, 4)
    print(json.dumps({lib: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)),
                            "ms": [round(float(x), 4) for x in v],
                            "TBps": ab / (np.median(v) * 1e-3) / 1e12, "checksum": chk[lib]}
                      for lib, v in res.items()}))

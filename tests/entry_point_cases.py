"""The case table of tests/test_gpu_dirty_buffers.py and tests/test_gpu_side_stream.py (a test helper, not
a conftest): every entry point of dpt_hip at the smallest shapes that reach each of its code paths.

A ``Case`` is three functions.  ``inputs(seed)`` builds one valid set of device inputs (dict name ->
tensor; another seed gives another valid set of the same shapes and ranges: the decoys of the side-stream
test; a packed weight blob is an input where the entry point takes one).  ``prepare(inp)`` builds what
lives across calls (a trainer, a resident dataset, a packed model) around those tensors, so that copying
over them later changes what the binding reads.  ``call(obj, inp, dirty)`` runs the binding(s) and returns
the documented outputs (dict name -> tensor); ``dirty(t)`` fills a workspace the caller owns with the
pattern under test (a no-op outside the dirty-buffer test).  ``tuning`` lists (setter, value, default).

No case synchronises the host, copies from host memory inside ``call`` or reads a result back: the
side-stream test asserts that.  (LinUCB takes its arm features from the host, so that one case has
``side=False``: it runs in the dirty-buffer test only.)"""
import contextlib
import ctypes
import functools

import numpy as np
import torch


class Case:
    def __init__(self, name, inputs, call, prepare=None, tuning=(), side=True):
        self.name, self.inputs, self.call, self.prepare, self.side = name, inputs, call, prepare, side
        self._tuning = tuple(tuning)

    @contextlib.contextmanager
    def tuning(self):
        try:
            for setter, value, _ in self._tuning:
                setter(value)
            yield
        finally:
            for setter, _, default in self._tuning:
                setter(default)

    def __repr__(self):
        return self.name


CASES = []


def case(name, inputs, call, prepare=None, tuning=(), side=True):
    CASES.append(Case(name, inputs, call, prepare, tuning, side))


def ids():
    return [c.name for c in CASES]


def as_bytes(out):
    """{name: uint8 host copy} of a dict of output tensors (NaN != NaN, so results are compared as bytes)"""
    return {k: v.contiguous().view(torch.uint8).cpu() for k, v in out.items() if v is not None}


def same_bytes(a, b):
    """the names whose bytes differ (a missing name differs)"""
    return [k for k in sorted(set(a) | set(b)) if k not in a or k not in b or a[k].shape != b[k].shape
            or not torch.equal(a[k], b[k])]


def dev(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda")


def f32(x):
    return dev(x, torch.float32)


def f64(x):
    return dev(x, torch.float64)


def i32(x):
    return dev(x, torch.int32)


def i64(x):
    return dev(x, torch.int64)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- models
@functools.lru_cache(maxsize=None)
def golden_model(name):
    """the DeviceModel of tests/golden/forward_<name>.npz (width 32, 4 layers) and its config"""
    import dpt_hip
    from conftest import golden
    g = golden(f"forward_{name}.npz")
    w = {k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w/")}
    H, sd, A, L, _ = (int(x) for x in g["cfg"])
    m = dpt_hip.DeviceModel(w, L, sd, A, 4 * (1 + H))
    torch.cuda.synchronize()
    return m, sd, A


@functools.lru_cache(maxsize=None)
def transformer(E, L, H, sd, A, seed, dropout=0.0, test=False):
    """a perturbed models.net.Transformer on the device (the construction of test_gpu_train*.py)"""
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=L, n_embd=E, n_head=1, dropout=dropout,
                         test=test))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m.cuda()


@functools.lru_cache(maxsize=None)
def mdp_model(E, L, K, seed):
    import interactive_mdp_oracle as MO
    return MO.model(E, L, K, seed)[0].cuda().eval()


@functools.lru_cache(maxsize=None)
def image_model(E, seed, test=False):
    """test_gpu_image_step.make_model's ImageTransformer (state_dim 2, 4 actions, horizon 3, 2 layers)"""
    from models.net import ImageTransformer
    torch.manual_seed(seed)
    m = ImageTransformer(dict(horizon=3, state_dim=2, action_dim=4, n_layer=2, n_embd=E, n_head=1, shuffle=False,
                              dropout=0.0, test=test, store_gpu=False, image_size=25))
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn_like(q))
    m = m.cuda()
    return m.eval() if test else m


def blob_of(model, seed):
    """the model's packed blob (seed 0) or another valid blob of the same layout (the decoy)"""
    from dpt_hip import train as tr
    blob = tr.pack_params(tr.param_list(model), torch.device("cuda", torch.cuda.current_device()))
    if seed:
        g = torch.Generator(device="cpu").manual_seed(seed)
        blob = blob + 0.02 * torch.randn(blob.shape, generator=g).to(blob.device)
    return blob.contiguous()


def rs_of(seed, salt):
    return np.random.RandomState(1000 * salt + seed)


# ----------------------------------------------------------------------------- forward_window / decode_step
def _window_inputs(N, C, sd, A, salt):
    def inputs(seed):
        rs = rs_of(seed, salt)
        inp = dict(query=f32(rs.randint(0, 10, (N, sd))))
        if C:
            inp.update(cs=f32(rs.randint(0, 10, (N, C, sd))), ca=f32(np.eye(A)[rs.randint(0, A, (N, C))]),
                       cn=f32(rs.randint(0, 10, (N, C, sd))), cr=f32(rs.randint(0, 2, (N, C))))
        return inp
    return inputs


def _window_call(out_mode):
    def call(obj, inp, dirty):
        m = golden_model("darkroom")[0]
        if "cs" not in inp:
            return dict(logits=m.forward_window(inp["query"]))
        return dict(logits=m.forward_window(inp["query"], inp["cs"], inp["ca"], inp["cn"], inp["cr"],
                                            out_mode=out_mode))
    return call


def _add_window_cases():
    import dpt_hip
    for C in (0, 16, 17):
        for out_mode in (0, 1):
            if C == 0 and out_mode == 1:
                continue  # no context rows: nothing runs
            case(f"forward_window-C{C}-mode{out_mode}", _window_inputs(3, C, 2, 5, 1), _window_call(out_mode))
    for out_mode in (0, 1):
        case(f"forward_window-decode-C17-mode{out_mode}", _window_inputs(3, 17, 2, 5, 1), _window_call(out_mode),
             tuning=[(dpt_hip.set_prefill, False, True)])

    def dec_inputs(seed):
        rs = rs_of(seed, 2)
        tok = np.zeros((10, 3, 10))
        tok[:, :, :2] = rs.randint(0, 10, (10, 3, 2))
        tok[1:, :, 2:7] = np.eye(5)[rs.randint(0, 5, (9, 3))]
        tok[1:, :, 7:9] = rs.randint(0, 10, (9, 3, 2))
        tok[1:, :, 9] = rs.randint(0, 2, (9, 3))
        return dict(tokens=f32(tok))

    def dec_call(obj, inp, dirty):
        m = golden_model("darkroom")[0]
        kv = torch.empty(m.kv_numel(3, 10), dtype=torch.float32, device="cuda")
        dirty(kv)
        return {f"logits{p}": m.decode_step(kv, 10, p, inp["tokens"][p]) for p in range(10)}
    case("decode_step-pos0..9", dec_inputs, dec_call)


# ----------------------------------------------------------------------------- rollout_bandit
def _bandit_inputs(N, H, A, salt, bern=False):
    def inputs(seed):
        rs = rs_of(seed, salt)
        return dict(means=f64(rs.uniform(0, 1, (N, A))), uniforms=f64(rs.uniform(size=(H, N))),
                    noise=f64(rs.uniform(size=(H, N)) if bern else rs.normal(size=(H, N))))
    return inputs


BANDIT_OUT = ("actions", "rewards", "arm_value", "logits")


def _add_bandit_cases():
    import dpt_hip
    N, H, A = 9, 70, 5

    def call_for(bern, own_kv):
        def call(obj, inp, dirty):
            m = golden_model("bandit5")[0]
            kv = None
            if own_kv:  # the caller's workspace: a view into a larger allocation
                kv = torch.empty(m.kv_numel(N, H) + 64, dtype=torch.float32, device="cuda")
                dirty(kv)
                kv = kv[32:]
            o = m.rollout_bandit(inp["means"], H, 0.3, True, dpt_hip.BANDIT_BERNOULLI if bern else
                                 dpt_hip.BANDIT_GAUSSIAN, uniforms=inp["uniforms"], noise=inp["noise"],
                                 want_logits=True, kvcache=kv)
            return {k: o[k] for k in BANDIT_OUT}
        return call
    bits = lambda b: (dpt_hip.set_ycache_bits, b, 24)  # noqa: E731
    tile = lambda t: (dpt_hip.set_decode_tile, t, 8)  # noqa: E731
    variants = [("base", [], False, False), ("own-kv", [], False, True), ("ycache32", [bits(32)], False, True),
                ("tile16", [tile(16)], False, True), ("tile16-ycache32", [tile(16), bits(32)], False, False),
                ("budget0", [(dpt_hip.set_cache_budget, 0, 224 << 20)], False, True),
                ("bernoulli", [], True, True)]
    for name, tuning, bern, own in variants:
        case(f"rollout_bandit-{name}", _bandit_inputs(N, H, A, 3, bern), call_for(bern, own), tuning=tuning)

    def philox_call(obj, inp, dirty):  # the library's own draws, greedy and sampled
        m = golden_model("bandit5")[0]
        out = {}
        for sample in (True, False):
            o = m.rollout_bandit(inp["means"], H, 0.3, sample, seed=77, first_task=5, counter=3, want_logits=True)
            out.update({f"{k}-{int(sample)}": o[k] for k in BANDIT_OUT})
        return out
    case("rollout_bandit-philox", lambda seed: dict(means=f64(rs_of(seed, 4).uniform(0, 1, (N, A)))), philox_call)


# ----------------------------------------------------------------------------- rollout_darkroom (+ episode)
def _add_darkroom_cases():
    import dpt_hip
    N = 5

    def inputs_for(Heps, horizon, dim):
        def inputs(seed):
            rs = rs_of(seed, 5)
            return dict(goals=i32(rs.randint(0, dim, (N, 2))), uniforms=f64(rs.uniform(size=(Heps * horizon, N))),
                        perms=i32(np.stack([rs.permutation(5) for _ in range(N)])))
        return inputs

    def call_for(Heps, horizon, R, dim):
        def call(obj, inp, dirty):
            m = golden_model("darkroom")[0]
            o = m.rollout_darkroom(inp["goals"], Heps, horizon, R, dim=dim, perms=inp["perms"], sample=True,
                                   uniforms=inp["uniforms"], want_actions=True, want_logits=True, want_forwards=True)
            return {k: o[k] for k in ("returns", "actions", "logits", "forwards")}
        return call
    ws = lambda on: (dpt_hip.set_darkroom_workspace, on, True)  # noqa: E731
    memo = lambda on: (dpt_hip.set_darkroom_memo, on, True)  # noqa: E731
    for (Heps, horizon, R) in ((3, 30, 2), (2, 130, 1)):
        for w in (True, False):
            for mm in (True, False):
                case(f"rollout_darkroom-{Heps}x{horizon}-R{R}-ws{int(w)}-memo{int(mm)}", inputs_for(Heps, horizon, 10),
                     call_for(Heps, horizon, R, 10), tuning=[ws(w), memo(mm)])
    case("rollout_darkroom-3x30-R2-dim12-ws0", inputs_for(3, 30, 12), call_for(3, 30, 2, 12), tuning=[ws(False)])

    import episode_rollout_cases as EC
    for name in ("K17", "K129"):
        K, n, dim, _ = EC.TABLE[name]

        def ep_inputs(seed, K=K, n=n, dim=dim):
            rs = rs_of(seed, 6)
            return dict(goals=i32(rs.randint(0, dim, (n, 2))), uniforms=f64(rs.uniform(size=(K - 1, n))),
                        perm=i32(np.stack([rs.permutation(5) for _ in range(n)])))

        def ep_prepare(inp, K=K):
            m = mdp_model(32, EC.LAYERS, K, 2000 + K)
            m.device_model()  # packs and uploads the weights (synchronises)
            return m

        def ep_call(m, inp, dirty, K=K, dim=dim):
            rec, ret, lg = dpt_hip.rollout_darkroom_episode(m, inp["goals"], K, dim, True, perm=inp["perm"],
                                                            uniforms=inp["uniforms"], logits=True)
            return dict(rec, returns=ret, logits=lg)
        case(f"rollout_darkroom_episode-{name}", ep_inputs, ep_call, ep_prepare)


# ----------------------------------------------------------------------------- classical policies
def _add_policy_cases():
    import dpt_hip
    N, A, H = 8, 5, 20
    ts = dict(ts_std=0.3, ts_prior_mean=0.5, ts_prior_var=1 / 12.0)
    arms = np.random.RandomState(8).normal(size=(A, 2))  # LinUCB's arm features (host: the binding reads their shape)
    table = [("emp", dpt_hip.POLICY_EMP, dict(online=True), True), ("ucb", dpt_hip.POLICY_UCB, dict(c=1.0), True),
             ("thompson-sampled", dpt_hip.POLICY_THOMPSON, dict(sample=True, **ts), True),
             ("thompson-vote", dpt_hip.POLICY_THOMPSON, dict(sample=False, seed=21, **ts), True),
             ("linucb-d2", dpt_hip.POLICY_LINUCB, dict(c=1.0, arms=arms, seed=22), False)]
    for name, pol, kw, side in table:
        for C in (0, 7):
            def inputs(seed, C=C, name=name):
                rs = rs_of(seed, 7)
                inp = dict(means=f64(rs.uniform(0, 1, (N, A))), noise=f64(rs.normal(size=(H, N))))
                if name == "thompson-sampled":
                    inp["policy_noise"] = f64(rs.normal(size=(H, N, A)))
                if C:
                    inp.update(ctx_actions=i32(rs.randint(0, A, (N, C))), ctx_rewards=f64(rs.normal(0.5, 0.5, (N, C))))
                return inp

            def call(obj, inp, dirty, pol=pol, kw=kw):
                o = dpt_hip.rollout_policy(pol, inp["means"], H, 0.3, noise=inp["noise"],
                                           policy_noise=inp.get("policy_noise"), ctx_actions=inp.get("ctx_actions"),
                                           ctx_rewards=inp.get("ctx_rewards"), **kw)
                return {k: o[k] for k in ("actions", "rewards", "arm_value")}
            case(f"rollout_policy-{name}-C{C}", inputs, call, side=side)


# ----------------------------------------------------------------------------- element-wise ops, data generation, statistics
def _add_small_cases():
    import dpt_hip
    from dpt_hip import _lib
    N, A = 70, 5

    case("select_action", lambda seed: dict(logits=f32(rs_of(seed, 9).normal(size=(N, A))),
                                            uniforms=f64(rs_of(seed, 10).uniform(size=N))),
         lambda obj, inp, dirty: dict(sampled=dpt_hip.select_action(inp["logits"], True, 0.7, uniforms=inp["uniforms"]),
                                      greedy=dpt_hip.select_action(inp["logits"], False),
                                      philox=dpt_hip.select_action(inp["logits"], True, seed=5, counter=2, first_task=9)))

    def bs_call(obj, inp, dirty):
        r, v = dpt_hip.bandit_step(inp["means"], inp["action"], 0.3, noise=inp["noise"])
        rb, vb = dpt_hip.bandit_step(inp["means"], inp["action"], 0.3, dpt_hip.BANDIT_BERNOULLI, seed=4, counter=1)
        return dict(r=r, v=v, rb=rb, vb=vb)
    case("bandit_step", lambda seed: dict(means=f64(rs_of(seed, 11).uniform(0, 1, (N, A))),
                                          action=i32(rs_of(seed, 12).randint(0, A, N)),
                                          noise=f64(rs_of(seed, 13).normal(size=N))), bs_call)

    def dr_inputs(seed):
        rs = rs_of(seed, 14)
        return dict(state=i32(rs.randint(0, 10, (N, 2))), action=i32(rs.randint(0, 5, N)),
                    goal=i32(rs.randint(0, 10, (N, 2))), perm=i32(np.stack([rs.permutation(5) for _ in range(N)])))

    def dr_call(obj, inp, dirty):
        ns, r = dpt_hip.darkroom_step(inp["state"], inp["action"], inp["goal"], inp["perm"], dim=10)
        ns2, r2 = dpt_hip.darkroom_step(inp["state"], inp["action"], inp["goal"], None, dim=10)
        return dict(ns=ns, r=r, ns2=ns2, r2=r2)
    case("darkroom_step", dr_inputs, dr_call)
    case("darkroom_opt_action", dr_inputs,
         lambda obj, inp, dirty: dict(a=dpt_hip.darkroom_opt_action(inp["state"], inp["goal"], inp["perm"]),
                                      b=dpt_hip.darkroom_opt_action(inp["state"], inp["goal"])))

    def rb_inputs(seed):
        rs = rs_of(seed, 15)
        return dict(means=f64(rs.uniform(0, 1, (N, A))), probs=f64(rs.dirichlet(np.ones(A), N)))

    def rb_call(obj, inp, dirty):
        a, r = dpt_hip.rollin_bandit(inp["means"], inp["probs"], 13, 0.3, seed=31, first_task=2)
        return dict(actions=a, rewards=r)
    case("rollin_bandit", rb_inputs, rb_call)

    def rd_call(obj, inp, dirty):
        return dpt_hip.rollin_darkroom(inp["goal"], 13, dim=10, perm=inp["perm"], seed=33, first_task=1)
    case("rollin_darkroom", dr_inputs, rd_call)

    for (n, H) in ((3, 7), (67, 130)):
        def rg_inputs(seed, n=n, H=H):
            rs = rs_of(seed, 16)
            return dict(arm_value=f64(rs.uniform(0, 1, (n, H))), opt=f64(rs.uniform(1, 2, n)),
                        mean=f64(rs.uniform(0, 1, (2, H))))

        def rg_call(obj, inp, dirty, n=n, H=H):
            # the ctypes-level call on the caller's workspace, filled directly, and the binding's own
            k = ctypes.c_int64()
            _lib.call("dpt_regret_workspace_numel", n, H, ctypes.byref(k))
            ws = torch.empty(k.value, dtype=torch.float64, device="cuda")
            dirty(ws)
            sums = torch.empty((2, H), dtype=torch.float64, device="cuda")
            _lib.call("dpt_regret_moments", _p(inp["arm_value"]), _p(inp["opt"]), n, H, _lib.REGRET_SUMS, None, _p(ws),
                      _p(sums), _stream())
            return dict(sums=sums, centred=dpt_hip.regret_moments(inp["arm_value"], inp["opt"], _lib.REGRET_CENTRED,
                                                                  inp["mean"]))
        case(f"regret_moments-{n}x{H}", rg_inputs, rg_call)


# ----------------------------------------------------------------------------- explore-then-exploit evaluation
def _add_recommend_cases():
    import dpt_hip
    from dpt_hip import train as tr
    N, T, A = 67, 7, 5

    def rc_inputs(seed):
        rs = rs_of(seed, 17)
        return dict(logits=f32(rs.normal(size=(N, T, A))), means=f64(rs.uniform(0, 1, (N, A))),
                    targets=i64(rs.randint(0, A, N)), actions=i32(rs.randint(0, A, (N, T - 1))),
                    rewards=f64(rs.normal(0.5, 0.5, (N, T - 1))))
    keys = ("greedy_arm", "greedy_value", "expected_value", "p_opt")

    def rc_call(obj, inp, dirty):
        o = dpt_hip.recommend_curve(inp["logits"], inp["means"], inp["targets"])
        return {k: o[k] for k in keys}
    case("recommend_curve", rc_inputs, rc_call)

    def er_call(obj, inp, dirty):
        o = dpt_hip.empirical_recommend(inp["actions"], inp["rewards"], inp["means"])
        return dict(emp_arm=o["emp_arm"], emp_value=o["emp_value"])
    case("empirical_recommend", rc_inputs, er_call)

    n, H = 7, 6
    for E in (32, 18):
        def ee_inputs(seed, E=E):
            rs = rs_of(seed, 18)
            return dict(blob=blob_of(transformer(E, 2, H, 1, A, 40 + E), seed), means=f64(rs.uniform(0, 1, (n, A))),
                        actions=i32(rs.randint(0, A, (n, H))), rewards=f64(rs.normal(0.5, 0.5, (n, H))),
                        targets=i64(rs.randint(0, A, n)))

        def ee_call(obj, inp, dirty, E=E):
            o = tr.exploit_curve(transformer(E, 2, H, 1, A, 40 + E), inp["actions"], inp["rewards"], inp["means"],
                                 targets=inp["targets"], chunk=3, blob=inp["blob"], want_logits=True)
            return {k: o[k] for k in keys + ("logits",)}
        case(f"exploit_eval-E{E}-chunk3", ee_inputs, ee_call)


# ----------------------------------------------------------------------------- training forward + backward
SD, A_TR, L_TR = 2, 5, 2
F_TR = 2 * SD + A_TR + 1


def _tokens(rs, B, T):
    tok = np.zeros((B, T, F_TR))
    tok[:, :, :SD] = rs.randint(0, 10, (B, T, SD))
    if T > 1:
        tok[:, 1:, SD:SD + A_TR] = np.eye(A_TR)[rs.randint(0, A_TR, (B, T - 1))]
        tok[:, 1:, SD + A_TR:2 * SD + A_TR] = rs.randint(0, 10, (B, T - 1, SD))
        tok[:, 1:, -1] = rs.normal(0.5, 0.5, (B, T - 1))
    return tok


def _add_train_cases():
    from dpt_hip import _lib
    from dpt_hip import train as tr
    shapes = [(32, 1, 2), (32, 17, 3), (32, 65, 2), (16, 17, 3), (64, 65, 2), (18, 38, 3), (48, 17, 2)]
    table = [(E, T, B, mode, 0.0) for (E, T, B) in shapes for mode in ("full", "last_only", "last_loss")]
    table += [(32, 17, 3, "full", 0.1), (18, 17, 3, "full", 0.1)]
    for E, T, B, mode, p in table:
        model = functools.partial(transformer, E, L_TR, T - 1, SD, A_TR, 50 + E, p)

        def inputs(seed, E=E, T=T, B=B, model=model):
            rs = rs_of(seed, 19)
            return dict(blob=blob_of(model(), seed), tokens=f32(_tokens(rs, B, T)),
                        dpreds=f32(rs.normal(size=(B, T, A_TR))))

        def call(obj, inp, dirty, E=E, T=T, B=B, mode=mode, p=p):
            flags = {"full": 0, "last_only": tr.FORWARD_ONLY | tr.LAST_ONLY, "last_loss": tr.LAST_LOSS}[mode]
            d = tr.desc(L_TR, E, SD, A_TR, 4 * T, B, T, flags, dropout=p, seed=1234)
            # the ctypes-level forward on the caller's workspace, filled directly
            ws = torch.empty(tr._numel("dpt_train_workspace_numel", d), dtype=torch.float32, device="cuda")
            dirty(ws)
            preds = torch.empty((B, T, A_TR), dtype=torch.float32, device="cuda")
            _lib.call("dpt_train_forward", ctypes.byref(d), _p(inp["blob"]), _p(inp["tokens"]), _p(ws), _p(preds),
                      _stream())
            if mode == "last_only":
                return dict(preds_last=preds[:, -1])
            dblob = tr.backward(d, inp["blob"], inp["tokens"], ws, inp["dpreds"])
            if mode == "last_loss":  # only preds[:, T - 1] is documented as written (window 1 runs the full path)
                return dict(preds_last=preds[:, -1], dblob=dblob)
            return dict(preds=preds, dblob=dblob)
        case(f"train-E{E}-T{T}-B{B}-{mode}" + ("-dropout" if p else ""), inputs, call)

    for E in (32, 18):
        T, B = 7, 2
        model = functools.partial(transformer, E, L_TR, T - 1, SD, A_TR, 50 + E, 0.0)

        def em_inputs(seed, E=E, model=model):
            rs = rs_of(seed, 20)
            return dict(blob=blob_of(model(), seed), embeds=f32(rs.normal(size=(B, T, E))),
                        dpreds=f32(rs.normal(size=(B, T, A_TR))))

        def em_call(obj, inp, dirty, E=E):
            d = tr.desc(L_TR, E, SD, A_TR, 4 * T, B, T)
            preds, ws = tr.forward_embeds(d, inp["blob"], inp["embeds"])
            dblob, dembeds = tr.backward_embeds(d, inp["blob"], ws, inp["dpreds"])
            return dict(preds=preds, dblob=dblob, dembeds=dembeds)
        case(f"train_embeds-E{E}-T{T}-B{B}", em_inputs, em_call)

    def aw_inputs(seed):
        rs = rs_of(seed, 21)
        n = 1003
        return dict(blob=f32(rs.normal(size=n)), grad=f32(rs.normal(size=n)), m=f32(0.1 * rs.normal(size=n)),
                    v=f32(0.01 * rs.uniform(size=n)))

    def aw_call(obj, inp, dirty):
        opt = _lib.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 3)
        _lib.call("dpt_adamw_step", _p(inp["blob"]), _p(inp["grad"]), _p(inp["m"]), _p(inp["v"]), inp["blob"].numel(),
                  ctypes.byref(opt), _stream())
        return dict(blob=inp["blob"], m=inp["m"], v=inp["v"])
    case("adamw_step", aw_inputs, aw_call)


# ----------------------------------------------------------------------------- image front end
def _add_image_cases():
    import dpt_hip
    from dpt_hip import _lib
    from dpt_hip import train as tr
    sd, A = 2, 4
    G = sd + A + 1
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])

    def images(rs, n):
        return ((rs.uniform(0, 1, (n, 25, 25, 3)) - mean) / std).transpose(0, 3, 1, 2)

    def front_blob(E, seed):
        m = image_model(E, 60 + E)
        blob = dpt_hip.pack_front({k: v.detach() for k, v in m.state_dict().items() if k in dpt_hip.FRONT_KEYS})
        if seed:
            g = torch.Generator(device="cpu").manual_seed(seed)
            blob = blob + 0.02 * torch.randn(blob.shape, generator=g).to(blob.device)
        return blob.contiguous()

    for rows, E in ((1, 32), (5, 32), (1, 18), (5, 18)):
        def fr_inputs(seed, rows=rows, E=E):
            rs = rs_of(seed, 22)
            return dict(blob=front_blob(E, seed), images=f32(images(rs, rows)), feats=f32(rs.normal(size=(rows, G))),
                        dembeds=f32(rs.normal(size=(rows, E))))

        def fr_call(obj, inp, dirty, rows=rows, E=E):
            d = tr.image_desc(rows, sd, A, E)
            embeds, ws = tr.front_forward(d, inp["blob"], inp["images"], inp["feats"])
            dblob = tr.front_backward(d, inp["blob"], inp["images"], inp["feats"], ws, inp["dembeds"])
            fo = tr.image_desc(rows, sd, A, E, flags=tr.FORWARD_ONLY)
            return dict(embeds=embeds, dblob=dblob,
                        embeds_fo=tr.front_forward(fo, inp["blob"], inp["images"], inp["feats"])[0])
        case(f"image_front-rows{rows}-E{E}", fr_inputs, fr_call)

    def nm_inputs(seed):
        rs = rs_of(seed, 23)
        return dict(raw64=f64(rs.uniform(0, 1, (7, 25, 25, 3))), raw32=f32(rs.uniform(0, 1, (3, 25, 25, 3))))
    case("image_normalize", nm_inputs,
         lambda obj, inp, dirty: dict(a=tr.normalize_images(inp["raw64"]), b=tr.normalize_images(inp["raw32"])))

    n, H = 5, 3

    def data_inputs(seed):
        rs = rs_of(seed, 24)
        return dict(query_states=f32(rs.normal(size=(n, sd))), context_states=f32(rs.normal(size=(n, H, sd))),
                    context_actions=f32(np.eye(A)[rs.randint(0, A, (n, H))]), context_rewards=f32(rs.normal(size=(n, H))),
                    optimal_actions=f32(np.eye(A)[rs.randint(0, A, n)]), query_images=f32(images(rs, n)),
                    context_images=f32(images(rs, n * H).reshape(n, H, 3, 25, 25)),
                    index=i64(rs.permutation(n)[:4]), perm=i64(np.stack([rs.permutation(H) for _ in range(4)])))
    data_keys = tr.IMAGE_DATA_KEYS + ("query_images", "context_images")

    def pk_prepare(inp):
        return tr.DeviceImageData.from_arrays({k: inp[k] for k in data_keys})

    def pk_call(dd, inp, dirty):
        B = 4
        d = tr.desc(2, 32, sd, A, 4 * (1 + H), B, 1 + H)
        out = dict(images=torch.empty((B, 1 + H, 3, 25, 25), dtype=torch.float32, device="cuda"),
                   feats=torch.empty((B, 1 + H, G), dtype=torch.float32, device="cuda"),
                   targets=torch.empty((B, A), dtype=torch.float32, device="cuda"))
        _lib.call("dpt_image_pack_batch", ctypes.byref(d), ctypes.byref(dd.struct), _p(inp["index"]), _p(inp["perm"]), B,
                  _p(out["images"]), _p(out["feats"]), _p(out["targets"]), _stream())
        return out
    case("image_pack_batch", data_inputs, pk_call, pk_prepare)

    Bact, C, hw = 3, 2, (32, 40)

    def act_inputs(seed):
        rs = rs_of(seed, 25)
        return dict(context_images=f32(images(rs, Bact * C).reshape(Bact, C, 3, 25, 25)),
                    context_states=f32(rs.normal(size=(Bact, C, sd))),
                    context_actions=f32(np.eye(A)[rs.randint(0, A, (Bact, C))]),
                    context_rewards=f32(rs.normal(size=(Bact, C))),
                    frames=dev(rs.randint(0, 256, (Bact,) + hw + (3,)), torch.uint8),
                    query_states=f32(rs.normal(size=(Bact, sd))), uniforms=f64(rs.uniform(size=Bact)))

    def act_prepare(inp):
        sess = dpt_hip.ImageActSession(image_model(32, 70, test=True), Bact, hw)
        sess._blobs()
        return sess

    def act_call(sess, inp, dirty):
        sess.set_context({k: inp[k] for k in ("context_images", "context_states", "context_actions", "context_rewards")})
        a = sess.act(inp["frames"], inp["query_states"], True, uniforms=inp["uniforms"])
        out = dict(actions=a, logits=sess.logits.clone(), obs=sess.obs.clone(), embeds=sess.embeds.clone())
        dirty(sess.ws)
        out["actions2"] = sess.act(inp["frames"], inp["query_states"], False)  # a second step on the same context
        out["logits2"] = sess.logits.clone()
        return out
    case("image_act-set_context+act_step", act_inputs, act_call, act_prepare)

    # the image trainer's fused step: two steps, the second batch smaller, then the test loss
    for E in (32, 18):
        def it_inputs(seed, E=E):
            m = image_model(E, 80 + E)
            front, trunk = tr.pack_image_params(tr.image_param_list(m), (2 * sd + A + 1) * E + E, torch.device("cuda"))
            if seed:
                g = torch.Generator(device="cpu").manual_seed(seed)
                front = front + 0.02 * torch.randn(front.shape, generator=g).to(front.device)
                trunk = trunk + 0.02 * torch.randn(trunk.shape, generator=g).to(trunk.device)
                trunk[:(2 * sd + A + 1) * E + E] = 0
            inp = data_inputs(seed)
            inp.update(front=front.contiguous(), trunk=trunk.contiguous(), index2=inp["index"][:2].clone(),
                       perm2=inp["perm"][:2].clone())
            return inp

        def it_prepare(inp, E=E):
            t = tr.ImageTrainer(image_model(E, 80 + E), lr=1e-3)
            t.front.blob, t.trunk.blob = inp["front"], inp["trunk"]
            return t, tr.DeviceImageData.from_arrays({k: inp[k] for k in data_keys})

        def it_call(obj, inp, dirty):
            t, dd = obj
            t.step(dd, inp["index"], inp["perm"], seed=5)
            dirty(t._ws)
            t.step(dd, inp["index2"], inp["perm2"], seed=6)
            dirty(t._ws)
            t.eval_loss(dd, inp["index2"], None, seed=7)
            return dict(blob=t.blob, m=t.m, v=t.v, front_blob=t.front_blob, front_m=t.front_m, front_v=t.front_v,
                        loss=t.loss)
        case(f"image_trainer-E{E}", it_inputs, it_call, it_prepare)


# ----------------------------------------------------------------------------- generic-width rollout
def _add_generic_cases():
    from dpt_hip import train as tr
    N, H, A = 9, 70, 5
    for E, f32_env in ((16, False), (16, True), (18, False), (64, False), (64, True), (128, False)):
        model = functools.partial(transformer, E, 2, H, 1, A, 90 + E)

        def inputs(seed, model=model):
            rs = rs_of(seed, 26)
            return dict(blob=blob_of(model(), seed), means=f64(rs.uniform(0, 1, (N, A))),
                        uniforms=f64(rs.uniform(size=(H, N))), noise=f64(rs.normal(size=(H, N))),
                        env_actions=i32(rs.randint(0, A, (H, N))))

        def call(obj, inp, dirty, model=model, f32_env=f32_env):
            o = tr.rollout_bandit_generic(model(), inp["means"], H, 0.3, True, uniforms=inp["uniforms"],
                                          noise=inp["noise"], want_logits=True, f32=f32_env, blob=inp["blob"],
                                          env_actions=inp["env_actions"] if f32_env else None)
            return {k: o[k] for k in BANDIT_OUT + (("env_actions",) if f32_env else ())}
        case(f"rollout_bandit_generic-E{E}" + ("-f32-env_actions" if f32_env else ""), inputs, call)


# ----------------------------------------------------------------------------- fused trainers
def _add_trainer_cases():
    from dpt_hip import train as tr
    A = 5
    # Trainer.step / eval_loss on a resident dataset
    n, H, sd = 7, 6, 2
    for E in (32, 18):
        model = functools.partial(transformer, E, 2, H, sd, A, 100 + E)

        def ds_inputs(seed, model=model):
            rs = rs_of(seed, 27)
            return dict(blob=blob_of(model(), seed), query_states=f32(rs.randint(0, 10, (n, sd))),
                        context_states=f32(rs.randint(0, 10, (n, H, sd))),
                        context_actions=f32(np.eye(A)[rs.randint(0, A, (n, H))]),
                        context_next_states=f32(rs.randint(0, 10, (n, H, sd))),
                        context_rewards=f32(rs.normal(0.5, 0.5, (n, H))),
                        optimal_actions=f32(np.eye(A)[rs.randint(0, A, n)]), index=i64(rs.permutation(n)[:5]),
                        perm=i64(np.stack([rs.permutation(H) for _ in range(5)])), index2=i64(rs.permutation(n)[:3]))

        def ds_prepare(inp, model=model):
            t = tr.Trainer(model(), lr=1e-3)
            t.state.blob = inp["blob"]
            return t, tr.DeviceData({k: inp[k] for k in tr.DATA_KEYS})

        def ds_call(obj, inp, dirty):
            t, dd = obj
            t.step(dd, inp["index"], inp["perm"])
            dirty(t._ws)
            t.step(dd, inp["index2"])
            dirty(t._ws)
            t.eval_loss(dd, inp["index2"])
            return dict(blob=t.blob, m=t.m, v=t.v, loss=t.loss)
        case(f"trainer-E{E}", ds_inputs, ds_call, ds_prepare)

    # the on-policy bandit trainers: 9 envs, then 5, K = 12
    K = 12
    model = functools.partial(transformer, 32, 2, K, 1, A, 110)
    other = functools.partial(transformer, 32, 2, K, 1, A, 111)

    def bt_inputs(seed):
        rs = rs_of(seed, 28)
        return dict(blob=blob_of(model(), seed), blob2=blob_of(other(), seed + 1 if seed else 0),
                    means=f64(rs.uniform(0, 1, (9, A))), uniforms=f64(rs.uniform(size=(K - 1, 9))),
                    noise=f64(rs.normal(size=(K - 1, 9))), env_actions=i32(rs.randint(0, A, (K - 1, 9))),
                    means2=f64(rs.uniform(0, 1, (5, A))), uniforms2=f64(rs.uniform(size=(K - 1, 5))),
                    noise2=f64(rs.normal(size=(K - 1, 5))), env_actions2=i32(rs.randint(0, A, (K - 1, 5))))

    for chunk in (0, 3):
        def ia_prepare(inp, chunk=chunk):
            t = tr.InteractiveTrainer(model(), lr=1e-3, chunk=chunk)
            t.state.blob = inp["blob"]
            return t

        def ia_call(t, inp, dirty):
            a1, r1 = t.step(inp["means"], K, 0.3, "uniform", uniforms=inp["uniforms"], noise=inp["noise"])
            dirty(t._ws)
            a2, r2 = t.step(inp["means2"], K, 0.3, "bernoulli", seed=91)
            return dict(blob=t.blob, m=t.m, v=t.v, dblob=t.dblob, loss=t.loss, a1=a1, r1=r1, a2=a2, r2=r2)
        case(f"interactive_trainer-chunk{chunk}", bt_inputs, ia_call, ia_prepare)

    for chunk in (0, 3):
        def ee_prepare(inp, chunk=chunk):
            t = tr.ExploreExploitTrainer(model(), other(), lr=1e-3, chunk=chunk)
            t.explorer_state.blob, t.exploiter_state.blob = inp["blob"], inp["blob2"]
            return t

        def ee_call(t, inp, dirty):
            rec1 = t.step(inp["means"], K, 0.3, "uniform", 0.5, uniforms=inp["uniforms"], noise=inp["noise"],
                          env_actions=inp["env_actions"])
            dirty(t._ws)
            rec2 = t.step(inp["means2"], K, 0.3, "uniform", 0.5, seed=92)
            out = dict(loss=t.loss)
            for name, s in (("explorer", t.explorer_state), ("exploiter", t.exploiter_state)):
                out.update({f"{name}_blob": s.blob, f"{name}_m": s.m, f"{name}_v": s.v, f"{name}_dblob": s.dblob})
            out.update({f"rec1_{i}": x for i, x in enumerate(rec1)}, **{f"rec2_{i}": x for i, x in enumerate(rec2)})
            return out
        case(f"explore_exploit_trainer-chunk{chunk}", bt_inputs, ee_call, ee_prepare)

    # the interactive DarkRoom trainer in each loss mode (and the loss-free rollout)
    Km, dim = 6, 3
    mm = functools.partial(mdp_model, 32, 2, Km, 120)

    def md_inputs(seed):
        rs = rs_of(seed, 29)
        return dict(blob=blob_of(mm(), seed), goals=i32(rs.randint(0, dim, (5, 2))),
                    uniforms=f64(rs.uniform(size=(Km - 1, 5))), perm=i32(np.stack([rs.permutation(5) for _ in range(5)])),
                    goals2=i32(rs.randint(0, dim, (3, 2))))

    for loss, chunk in (("every", 0), ("last", 0), ("every", 2), ("last", 2)):
        def md_prepare(inp, loss=loss, chunk=chunk):
            t = tr.InteractiveMDPTrainer(mm(), lr=1e-3, chunk=chunk, loss=loss)
            t.state.blob = inp["blob"]
            return t

        def md_call(t, inp, dirty):
            rec1 = t.step(inp["goals"], Km, dim, True, perm=inp["perm"], uniforms=inp["uniforms"])
            dirty(t._ws)
            rec2 = t.step(inp["goals2"], Km, dim, True, seed=93)
            out = dict(blob=t.blob, m=t.m, v=t.v, dblob=t.dblob, loss=t.loss)
            out.update({f"rec1_{k}": v for k, v in rec1.items()}, **{f"rec2_{k}": v for k, v in rec2.items()})
            return out
        case(f"interactive_mdp_trainer-{loss}-chunk{chunk}", md_inputs, md_call, md_prepare)

    def mr_call(obj, inp, dirty):
        rec, ret = tr.rollout_darkroom_interactive(mm(), inp["goals"], Km, dim, True, perm=inp["perm"],
                                                   uniforms=inp["uniforms"], chunk=2, blob=inp["blob"])
        return dict(rec, returns=ret)
    case("rollout_darkroom_interactive-chunk2", md_inputs, mr_call)


_built = False


def build():
    """fill CASES (needs the built library; no device work)"""
    global _built
    if not _built:
        _built = True
        for add in (_add_window_cases, _add_bandit_cases, _add_darkroom_cases, _add_policy_cases, _add_small_cases,
                    _add_recommend_cases, _add_train_cases, _add_image_cases, _add_generic_cases, _add_trainer_cases):
            add()
    return CASES

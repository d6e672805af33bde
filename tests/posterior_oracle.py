"""numpy restatement of the Bayes posterior of the optimal action (include/dpt_hip.h, "Bayes posterior of the
optimal action"; csrc/dpt_posterior.hip): a test helper.  The definitions are the header's, in the header's
operation order, vectorised over the tasks and looping over the rows t = 0 .. H."""
import numpy as np

GAUSSIAN, BERNOULLI = 0, 1


def grid(G):
    return (np.arange(G) + 0.5) / G


def loglik(n, s, x, var, bandit_type):
    """l_a(i) for statistics n, s (..., 1) on the grid x (G), in the header's operation order"""
    if bandit_type == BERNOULLI:
        return s * np.log(x) + (n - s) * np.log1p(-x)
    return -((n * x) * x - (2 * s) * x) / ((2 * var) * var)


def weights_cdf(n, s, var, bandit_type, G):
    """w (N, A, G) and the mid-point CDF C (N, A, G) of arms with statistics n, s (N, A)"""
    ll = loglik(n[..., None], s[..., None], grid(G), var, bandit_type)
    e = np.exp(ll - ll.max(-1, keepdims=True))
    w = e / e.sum(-1, keepdims=True)
    before = np.concatenate([np.zeros_like(w[..., :1]), np.cumsum(w, -1)[..., :-1]], -1)  # sum_{j<i} w(j)
    return w, before + w / 2


def posterior_from_stats(n, s, var, bandit_type, G):
    """post (N, A) of arms with statistics n, s (N, A)"""
    return normalise(*weights_cdf(np.asarray(n, np.float64), np.asarray(s, np.float64), var, bandit_type, G))


def normalise(w, C):
    """post (N, A) from w, C (N, A, G): u_a = sum_i w_a(i) prod_{b != a} C_b(i), normalised"""
    A = w.shape[1]
    pre = np.ones_like(C)   # prod_{b < a} C_b
    suf = np.ones_like(C)   # prod_{b > a} C_b
    for a in range(1, A):
        pre[:, a] = pre[:, a - 1] * C[:, a - 1]
    for a in range(A - 2, -1, -1):
        suf[:, a] = suf[:, a + 1] * C[:, a + 1]
    u = (w * (pre * suf)).sum(-1)
    return u / u.sum(-1, keepdims=True)


def prefix_stats(actions, rewards, A):
    """n, s (N, H + 1, A): pulls and reward sums (in pull order) of every arm after t = 0 .. H pulls; an
    action outside [0, A) adds to no arm"""
    actions, rewards = np.asarray(actions).reshape(len(actions), -1), np.asarray(rewards, np.float64)
    N, H = actions.shape
    n, s = np.zeros((N, H + 1, A)), np.zeros((N, H + 1, A))
    rows = np.arange(N)
    for t in range(H):
        n[:, t + 1], s[:, t + 1] = n[:, t], s[:, t]
        a = actions[:, t]
        ok = (a >= 0) & (a < A)
        n[rows[ok], t + 1, a[ok]] += 1.0
        s[rows[ok], t + 1, a[ok]] += rewards[ok, t]
    return n, s


def bandit_posterior(actions, rewards, A, var, bandit_type, G):
    """post (N, H + 1, A) float64: row t given the first t pulls.  An arm's w and C are functions of its own
    (n_a, s_a) alone, so between two rows only the pulled arm's are recomputed: the same values as
    ``posterior_from_stats`` on every row's statistics, at 1 / A of the exponentials."""
    n, s = prefix_stats(actions, rewards, A)
    actions = np.asarray(actions).reshape(len(n), -1)
    N, T = n.shape[:2]
    w, C = weights_cdf(n[:, 0], s[:, 0], var, bandit_type, G)
    post = np.empty((N, T, A))
    post[:, 0] = normalise(w, C)
    for t in range(1, T):
        a = actions[:, t - 1]
        ok = np.nonzero((a >= 0) & (a < A))[0]
        if len(ok):
            w[ok, a[ok]], C[ok, a[ok]] = weights_cdf(n[ok, t, a[ok]], s[ok, t, a[ok]], var, bandit_type, G)
        post[:, t] = normalise(w, C)
    return post


def darkroom_opt(x, y, gx, gy):
    """the expert action at (x, y) for goal (gx, gy), identity permutation (envs/darkroom_env.py:69-82)"""
    return np.where(x < gx, 0, np.where(x > gx, 1, np.where(y < gy, 2, np.where(y > gy, 3, 4))))


def darkroom_posterior(goals, query, next_states, rewards):
    """post (N, H + 1, 5) float64 and consistent (N, H + 1) int32"""
    goals = np.asarray(goals).reshape(-1, 2)
    query, rewards = np.asarray(query), np.asarray(rewards)
    N = len(query)
    rewards = rewards.reshape(N, -1)
    H = rewards.shape[1]
    next_states = np.asarray(next_states).reshape(N, H, 2)
    act = darkroom_opt(query[:, None, 0], query[:, None, 1], goals[None, :, 0], goals[None, :, 1])  # (N, K)
    alive = np.ones((N, len(goals)), bool)
    post, cons = np.zeros((N, H + 1, 5)), np.zeros((N, H + 1), np.int32)
    for t in range(H + 1):
        if t > 0:
            at_goal = (next_states[:, t - 1, None, :] == goals[None]).all(-1)
            alive &= (rewards[:, t - 1, None] != 0) == at_goal
        cnt = np.stack([(alive & (act == a)).sum(1) for a in range(5)], 1)
        cons[:, t] = cnt.sum(1)
        some = cons[:, t] > 0
        post[some, t] = cnt[some].astype(np.float64) / cons[some, t, None].astype(np.float64)
    return post, cons


def compare(post, logits, targets):
    """nll_model, nll_bayes, kl, entropy (N, T) float64: everything in float64 from the float32 logits"""
    post = np.asarray(post, np.float64)
    x = np.asarray(logits, np.float32).astype(np.float64)
    m = x.max(-1, keepdims=True)
    logq = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    tg = np.broadcast_to(np.asarray(targets).reshape(-1, 1, 1), post.shape[:2] + (1,))
    pos = post > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        logp = np.log(post)
        kl = np.where(pos, post * (logp - logq), 0.0).sum(-1)
        ent = -np.where(pos, post * logp, 0.0).sum(-1)
        nll_bayes = -np.take_along_axis(logp, tg, -1)[..., 0]
    return dict(nll_model=-np.take_along_axis(logq, tg, -1)[..., 0], nll_bayes=nll_bayes, kl=kl, entropy=ent)


def calibration_z(post, targets):
    """For the true posterior E[-log p(a* | D_t)] = E[entropy(p(. | D_t))].  The z-score of the per-task mean
    over t = 1 .. H of nll - entropy, over the tasks: (z, mean nll, mean entropy)."""
    c = compare(post, np.zeros(post.shape, np.float32), targets)
    d = (c["nll_bayes"] - c["entropy"])[:, 1:].mean(1)
    return d.mean() / (d.std(ddof=1) / np.sqrt(len(d))), c["nll_bayes"][:, 1:].mean(), c["entropy"][:, 1:].mean()


def bayes_floor(post, targets):
    """sum_{t=1..H} nll_bayes / H / n: the floor of train_fresh.py's test loss"""
    c = compare(post, np.zeros(post.shape, np.float32), targets)
    H = post.shape[1] - 1
    return c["nll_bayes"][:, 1:].sum() / H / len(post)


def adversarial_records(H, bandit_type, var, seed=0):
    """Six 5-arm tasks that stress the grid: near-ties of 1e-3, means at both ends of [0, 1], and a 96 %
    one-arm behaviour policy -> actions (6, H) int32, rewards (6, H)"""
    rs = np.random.RandomState(seed)
    means = np.array([[0.5, 0.501, 0.3, 0.2, 0.1], [0.999, 0.998, 0.5, 0.001, 0.0], [0.0, 0.001, 0.002, 0.5, 0.499],
                      [0.9, 0.899, 0.898, 0.897, 0.1], [0.001, 0.0, 0.002, 0.001, 0.0], [1.0, 0.999, 0.998, 0.5, 0.999]])
    probs = np.full((6, 5), 0.2)
    probs[3:] = 0.01
    probs[3, 0] = probs[4, 2] = probs[5, 4] = 0.96
    actions = np.stack([rs.choice(5, size=H, p=p) for p in probs]).astype(np.int32)
    mu = np.take_along_axis(means, actions, 1)
    if bandit_type == BERNOULLI:
        rewards = (rs.uniform(size=mu.shape) < mu).astype(np.float64)
    else:
        rewards = mu + var * rs.normal(size=mu.shape)
    return actions, rewards, means

"""numpy restatement of the linear bandit's Bayes posterior of the optimal arm at lin_d = 2 (include/dpt_hip.h,
"Linear bandit, lin_d = 2"; csrc/dpt_posterior_linear.hip): a test helper.  The definition is the header's, in
the header's operation order, in its pairwise O(A^2) form on every ray (the kernel walks the envelope instead),
vectorised over rows and rays.  ``dtype=np.longdouble`` evaluates the same definition in extended precision
(the float64 inputs and the float64 literal 2 pi taken exactly): the rounding floor of the float64 form."""
import numpy as np

TWO_PI = 6.283185307179586   # the header's literal
MIN_ANGLE = 2.0 ** -40       # a prior wedge narrower than this counts as empty


def prior(arms, dtype=np.float64):
    """post (A) before any valid pull: the angle of {psi : a = argmax_b x_b . (cos psi, sin psi)}, ties to the
    lower index, over 2 pi.  Arm a's set is the intersection over b != a of the open half-circles centred at
    theta_b = atan2 of x_a - x_b; relative to the first of them, delta_b in (-pi, pi], it is the arc of angle
    pi - max(0, max delta_b) + min(0, min delta_b)."""
    x = np.asarray(arms, np.float64).astype(dtype)
    A = len(x)
    pi = dtype(TWO_PI) / dtype(2)
    out = np.zeros(A, dtype)
    for a in range(A):
        first, hi, lo, dead = None, dtype(0), dtype(0), False
        for b in range(A):
            if b == a:
                continue
            d0, d1 = x[a, 0] - x[b, 0], x[a, 1] - x[b, 1]
            if d0 == 0 and d1 == 0:
                if b < a:
                    dead = True
                continue
            th = np.arctan2(d1, d0)
            if first is None:
                first = th
                continue
            dl = th - first
            if dl > pi:
                dl = dl - dtype(TWO_PI)
            elif dl <= -pi:
                dl = dl + dtype(TWO_PI)
            hi, lo = max(hi, dl), min(lo, dl)
        if dead:
            continue
        ang = dtype(TWO_PI) if first is None else (pi - hi) + lo
        out[a] = ang / dtype(TWO_PI) if ang >= MIN_ANGLE else 0
    return out


def prior_brute(arms, n=1 << 20):
    """the same by counting n directions (np.argmax: ties to the lower index)"""
    psi = TWO_PI * (np.arange(n) + 0.5) / n
    best = np.argmax(np.asarray(arms, np.float64) @ np.stack([np.cos(psi), np.sin(psi)]), 0)
    return np.bincount(best, minlength=len(arms)) / n


def moments(arms, actions, rewards, var, dtype=np.float64):
    """valid (N, H + 1) bool: a valid pull among the first t; m (N, H + 1, 2) and L = (L00, L10, L11)
    (N, H + 1, 3) of the posterior N(m, L L^T) of theta, in the header's operation order"""
    x = np.asarray(arms, np.float64).astype(dtype)
    actions = np.asarray(actions).reshape(len(actions), -1)
    rewards = np.asarray(rewards, np.float64).astype(dtype).reshape(actions.shape)
    N, H = actions.shape
    A = len(x)
    v2 = dtype(var) * dtype(var)
    st = np.zeros((N, H + 1, 5), dtype)
    valid = np.zeros((N, H + 1), bool)
    for t in range(H):
        a = actions[:, t]
        ok = (a >= 0) & (a < A)
        xa = x[np.where(ok, a, 0)]
        r = rewards[:, t]
        add = np.stack([(xa[:, 0] * xa[:, 0]) / v2, (xa[:, 0] * xa[:, 1]) / v2, (xa[:, 1] * xa[:, 1]) / v2,
                        (r * xa[:, 0]) / v2, (r * xa[:, 1]) / v2], 1)
        st[:, t + 1] = np.where(ok[:, None], st[:, t] + add, st[:, t])
        valid[:, t + 1] = valid[:, t] | ok
    sxx, sxy, syy, b0, b1 = (st[..., k] for k in range(5))
    l00, l01, l11 = dtype(2) + sxx, sxy, dtype(2) + syy
    det = l00 * l11 - l01 * l01
    s00, s01, s11 = l11 / det, -(l01 / det), l00 / det
    m = np.stack([s00 * b0 + s01 * b1, s01 * b0 + s11 * b1], -1)
    L00 = np.sqrt(s00)
    return valid, m, np.stack([L00, s01 / L00, dtype(1) / np.sqrt(l11)], -1)


def ray_masses(alpha, xl0, xl1, G, dtype=np.float64):
    """u (R, K): the sum over the G rays of every arm's mass, pairwise form; alpha, xl0, xl1 (R, K)"""
    phi = (dtype(TWO_PI) * (np.arange(G).astype(dtype) + dtype(0.5))) / dtype(G)
    c, s = np.cos(phi), np.sin(phi)
    R, K = alpha.shape
    u = np.empty((R, K), dtype)
    step = max(1, int(3e6) // (K * K * G))
    idx = np.arange(K)
    inf = dtype(np.inf)
    for r0 in range(0, R, step):
        al = alpha[r0:r0 + step]
        beta = xl0[r0:r0 + step, :, None] * c + xl1[r0:r0 + step, :, None] * s           # (r, K, G)
        db = beta[:, :, None, :] - beta[:, None, :, :]                                    # beta_a - beta_b
        da = (al[:, None, :] - al[:, :, None])[..., None]                                 # alpha_b - alpha_a
        with np.errstate(divide="ignore", invalid="ignore"):
            q = da / db
        lo = np.maximum(np.where(db > 0, q, -inf).max(2), 0)
        hi = np.where(db < 0, q, inf).min(2)
        lost = (db == 0) & ((da > 0) | ((da == 0) & (idx[None, :] < idx[:, None])[None, :, :, None]))
        mass = np.exp(-(lo * lo) / dtype(2)) - np.exp(-(hi * hi) / dtype(2))
        mass = np.where((hi <= lo) | lost.any(2), 0, mass)
        u[r0:r0 + step] = mass.sum(-1)
    return u


def linear_posterior(arms, actions, rewards, var, G, dtype=np.float64):
    """post (N, H + 1, A) in ``dtype``: row t given the first t pulls.  Rows before the first valid pull are
    the prior; an arm whose prior is 0 is dropped (every row exactly 0, and it bounds no other arm)."""
    x = np.asarray(arms, np.float64).astype(dtype)
    pr = prior(arms, dtype)
    keep = np.nonzero(pr > 0)[0]
    valid, m, L = moments(arms, actions, rewards, var, dtype)
    N, T = valid.shape
    post = np.zeros((N, T, len(x)), dtype)
    post[~valid] = pr
    if valid.any():
        mv, Lv = m[valid], L[valid]                                                       # (R, 2), (R, 3)
        xk = x[keep]
        alpha = xk[:, 0] * mv[:, :1] + xk[:, 1] * mv[:, 1:]
        xl0 = xk[:, 0] * Lv[:, :1] + xk[:, 1] * Lv[:, 1:2]
        xl1 = xk[:, 1] * Lv[:, 2:]
        u = ray_masses(alpha, xl0, xl1, G, dtype)
        tot = np.zeros(len(u), dtype)
        for k in range(u.shape[1]):   # in index order, as the kernel
            tot = tot + u[:, k]
        rows = np.zeros((len(u), len(x)), dtype)
        rows[:, keep] = u / tot[:, None]
        post[valid] = rows
    return post


def monte_carlo(arms, m, L, draws, seed):
    """(frequency of each arm being optimal, its standard error) under ``draws`` samples of theta ~ N(m, L L^T)"""
    z = np.random.RandomState(seed).normal(size=(draws, 2))
    th = np.stack([m[0] + L[0] * z[:, 0], m[1] + L[1] * z[:, 0] + L[2] * z[:, 1]], 1)
    f = np.bincount(np.argmax(th @ np.asarray(arms, np.float64).T, 1), minlength=len(arms)) / draws
    return f, np.sqrt(f * (1 - f) / draws)


def reference_arms(A, lin_d=2):
    """collect_data.py's arms"""
    return np.random.RandomState(seed=1234).normal(size=(A, lin_d)) / np.sqrt(lin_d)


def sample_records(arms, N, H, var, seed, thompson=False):
    """theta ~ N(0, I / 2), pulls uniform over the arms (or, ``thompson``, greedy on a posterior draw of the
    per-arm model with prior 0 / 1): actions (N, H) int32, rewards (N, H), theta (N, 2)"""
    rs = np.random.RandomState(seed)
    arms = np.asarray(arms, np.float64)
    A = len(arms)
    theta = rs.normal(size=(N, 2)) / np.sqrt(2)
    means = theta @ arms.T
    acts, rews = np.zeros((N, H), np.int32), np.zeros((N, H))
    n, s = np.zeros((N, A)), np.zeros((N, A))
    rows = np.arange(N)
    for t in range(H):
        if thompson:
            w = var * var / (var * var + n)
            mean = (1 - w) * np.where(n > 0, s / np.maximum(n, 1), 0.0)
            a = np.argmax(mean + rs.normal(size=(N, A)) / np.sqrt(1 + n / (var * var)), 1)
        else:
            a = rs.randint(0, A, N)
        r = means[rows, a] + var * rs.normal(size=N)
        acts[:, t], rews[:, t] = a, r
        n[rows, a] += 1
        s[rows, a] += r
    return acts, rews, theta


GPU_N, GPU_H, GPU_AS, GPU_GS, GPU_VARS = 7, 37, (2, 5, 20, 32), (64, 256), (0.3, 0.05)


def gpu_arms(A):
    """The arms of the GPU test at A arms.  A = 5: arm 2 is a copy of arm 0 (the tie goes to arm 0) and arm 3
    sits at the origin.  A >= 20 adds: arm 3 a copy of arm 1; arms 4, 5, 6 collinear on the hull's edge x = 2
    with arm 5 between the other two; arm 7 at the origin; arm 8 strictly inside the hull."""
    if A == 2:
        return np.array([[0.8, 0.3], [-0.5, 0.6]])
    x = np.random.RandomState(50 + A).normal(size=(A, 2)) / np.sqrt(2)
    if A == 5:
        x[2], x[3] = x[0], 0.0
        return x
    x[3] = x[1]
    x[4], x[5], x[6] = (2.0, 0.5), (2.0, -0.25), (2.0, -1.0)
    x[7] = 0.0
    x[8] = (0.1, 0.05)
    return x


def gpu_records(A, var):
    """actions (7, 37) int32 / rewards (7, 37) of the GPU test: task 0 has the out-of-range actions A and -1
    among its pulls, task 1 starts with four invalid actions (rows 1 .. 4 are still the prior), task 2 has every
    reward 0 (the mean stays at the apex), task 3 pulls one arm only (with var = 0.05: a concentrated,
    ill-conditioned precision), tasks 4 .. 6 are a uniform and two Thompson-like runs"""
    arms = gpu_arms(A)
    acts, rews, _ = sample_records(arms, GPU_N, GPU_H, var, 1000 * A + int(100 * var))
    ta, tr, _ = sample_records(arms, 2, GPU_H, var, 77 + A, thompson=True)
    acts[5:], rews[5:] = ta, tr
    acts[0, 0], acts[0, 5] = A, -1
    acts[1, :4] = (-1, A, A + 3, -7)
    rews[2] = 0.0
    acts[3] = A - 1
    return acts, rews

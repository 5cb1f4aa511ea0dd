"""Restatement of RCAEval's cMLP learner (``RCAEval/graph_construction/cmlp.py``: the model of
``cmlp()``, ``train_model_ista`` with penalty "H", ``prox_update``, ``regularize``, ``cMLP.GC``)
for this project's tests: plain torch tensor algebra with hand-derived gradients, all p networks
batched, dtype selectable. Not a copy of the reference's file.

Model, per series i (N = T - lag samples, K = p * lag inputs, A[n, c * lag + k] = X[n + k, c]):

    Z = A W1_i^T + b1_i        H = relu(Z)        o = H w2_i + b2_i        mse_i = mean((o - X[lag:, i])^2)

Gradient of ``sum_i mse_i + lam_ridge * sum_i |w2_i|^2`` with g = 2 (o - y) / N:

    dw2 = H^T g + 2 lam_ridge w2     db2 = sum g     dZ = (g w2^T) * [Z > 0]     db1 = sum_n dZ     dW1 = dZ^T A

One ISTA iteration: ``param -= lr * grad`` for every parameter, then (lam > 0) for k = 0..lag-1 in
turn, per (network, input series c) with n = |W1[:, c, :k+1]|:
``W1[:, c, :k+1] <- W1[:, c, :k+1] / max(n, lr lam) * max(n - lr lam, 0)``.

Parameters travel as a dict of batched tensors ``W1`` (p, hidden, p, lag), ``b1`` (p, hidden),
``w2`` (p, hidden), ``b2`` (p,), or packed as the engine takes them (``from_packed`` / ``to_packed``:
per network W1, b1, w2, b2 flattened, torch's own layouts).
"""
import numpy as np
import torch

VAR5_A = np.array([[0.5, 0.0, 0.0, 0.0, 0.0],
                   [0.6, 0.5, 0.0, 0.0, 0.0],
                   [0.0, -0.6, 0.5, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.5, 0.0],
                   [0.0, 0.0, 0.0, 0.5, 0.5]])


def _simulate(A, T, rng):
    p = A.shape[0]
    X = np.empty((T, p))
    X[0] = rng.standard_normal(p)
    for t in range(1, T):
        X[t] = A @ X[t - 1] + 0.5 * rng.standard_normal(p)
    return (X - X.mean(axis=0)) / X.std(axis=0, ddof=0)


def var5(T=150, seed=0):
    """The 5-series VAR(1) of the golden: A = 0.5 I with A[1, 0] = 0.6, A[2, 1] = -0.6, A[4, 3] = 0.5,
    x_0 ~ N(0, I), x_t = A x_{t-1} + 0.5 N(0, I); columns standardised (ddof 0). float64, T x 5."""
    return _simulate(VAR5_A, T, np.random.default_rng(seed))


def var(p, T, seed):
    """A stable sparse VAR(1) of any width: 0.5 on the diagonal, +-0.4 from series c - 1 to c."""
    rng = np.random.default_rng(seed)
    A = 0.5 * np.eye(p)
    for c in range(1, p):
        A[c, c - 1] = 0.4 if c % 2 else -0.4
    return _simulate(A, T, rng)


def random_params(p, lag, hidden, seed, scale=None):
    """Packed fp32 parameters, uniform in +-1 / sqrt(fan_in) like torch's default (own RNG)."""
    rng = np.random.default_rng(seed)
    nets = []
    for _ in range(p):
        a, b = (scale or 1.0 / np.sqrt(p * lag)), (scale or 1.0 / np.sqrt(hidden))
        nets += [rng.uniform(-a, a, hidden * p * lag), rng.uniform(-a, a, hidden), rng.uniform(-b, b, hidden),
                 rng.uniform(-b, b, 1)]
    return np.concatenate(nets).astype(np.float32)


def from_packed(params, p, lag, hidden, dtype=torch.float64):
    v = torch.as_tensor(np.asarray(params, dtype=np.float64).reshape(p, -1)).to(dtype)
    nw = hidden * p * lag
    assert v.shape[1] == nw + 2 * hidden + 1
    return {"W1": v[:, :nw].reshape(p, hidden, p, lag).clone(), "b1": v[:, nw:nw + hidden].clone(),
            "w2": v[:, nw + hidden:nw + 2 * hidden].clone(), "b2": v[:, nw + 2 * hidden].clone()}


def to_packed(P):
    p = P["W1"].shape[0]
    return torch.cat([P["W1"].reshape(p, -1), P["b1"], P["w2"], P["b2"].reshape(p, 1)], dim=1).reshape(-1).double().numpy()


def design(X, lag, dtype=torch.float64):
    """(A, Y): the lag-expanded inputs (N x p * lag) and the targets (N x p). X goes through
    float32 first, as the reference casts its frame."""
    X = torch.as_tensor(np.asarray(X, dtype=np.float64).astype(np.float32)).to(dtype)
    T, p = X.shape
    N = T - lag
    if N < 1:
        raise ValueError(f"cmlp_ref: no sample to fit (T={T} <= lag={lag})")
    A = torch.stack([X[k:k + N] for k in range(lag)], dim=2).reshape(N, p * lag)      # [n, c, k]
    return A, X[lag:]


def _forward(P, A, Y):
    p = P["W1"].shape[0]
    Z = torch.matmul(A, P["W1"].reshape(p, -1, A.shape[1]).transpose(1, 2)) + P["b1"][:, None, :]   # p, N, hidden
    H = torch.relu(Z)
    R = torch.einsum("inh,ih->in", H, P["w2"]) + P["b2"][:, None] - Y.T                            # p, N
    return Z, H, R


def smooth_losses(P, A, Y):
    """The p per-network MSEs."""
    return (_forward(P, A, Y)[2] ** 2).mean(dim=1)


def penalty(P):
    """sum over networks, input series and k of |W1[:, c, :k+1]| (``regularize``, "H", without lam)."""
    lag = P["W1"].shape[3]
    return sum(torch.sqrt((P["W1"][..., :k + 1] ** 2).sum(dim=(1, 3))).sum() for k in range(lag))


def prox(W1, thr):
    lag = W1.shape[3]
    for k in range(lag):
        n = torch.sqrt((W1[..., :k + 1] ** 2).sum(dim=(1, 3), keepdim=True))
        W1[..., :k + 1] = W1[..., :k + 1] / torch.clamp(n, min=thr) * torch.clamp(n - thr, min=0.0)
    return W1


def step(P, A, Y, lr, lam, lam_ridge):
    """One ISTA iteration in place."""
    p, N = P["W1"].shape[0], A.shape[0]
    Z, H, R = _forward(P, A, Y)
    g = 2.0 * R / N
    dw2 = torch.einsum("inh,in->ih", H, g) + 2.0 * lam_ridge * P["w2"]
    dZ = g[:, :, None] * P["w2"][:, None, :] * (Z > 0).to(Z.dtype)
    dW1 = torch.matmul(dZ.transpose(1, 2), A).reshape(P["W1"].shape)
    P["W1"] -= lr * dW1
    P["b1"] -= lr * dZ.sum(dim=1)
    P["w2"] -= lr * dw2
    P["b2"] -= lr * g.sum(dim=1)
    if lam > 0:
        prox(P["W1"], lr * lam)
    return P


def steps(X, params, k, lag=5, hidden=100, lr=5e-2, lam=0.002, lam_ridge=1e-2, dtype=torch.float64):
    """k iterations with no checks from packed parameters: (packed float64 array, per-network MSEs)."""
    A, Y = design(X, lag, dtype)
    P = from_packed(params, Y.shape[1], lag, hidden, dtype)
    for _ in range(k):
        step(P, A, Y, lr, lam, lam_ridge)
    return to_packed(P), smooth_losses(P, A, Y).double().numpy()


def losses_at(X, params, lag=5, hidden=100, dtype=torch.float64):
    """The per-network MSEs of packed parameters."""
    A, Y = design(X, lag, dtype)
    return smooth_losses(from_packed(params, Y.shape[1], lag, hidden, dtype), A, Y).double().numpy()


def train(X, params, max_iter, lag=5, hidden=100, lr=5e-2, lam=0.002, lam_ridge=1e-2, check_every=1000, lookback=5,
          dtype=torch.float64):
    """``train_model_ista``: dict with ``params`` (the restored best model, packed), ``last_params``
    (the last iterate), ``losses``, ``n_checks``, ``best_it``, ``last_it``. ValueError where the
    reference raises (its TypeErrors: no check ran, or a first check that is not below +inf)."""
    A, Y = design(X, lag, dtype)
    p = Y.shape[1]
    P = from_packed(params, p, lag, hidden, dtype)
    best_it, best_loss, best, losses, last_it = None, np.inf, None, [], max_iter - 1
    for it in range(max_iter):
        step(P, A, Y, lr, lam, lam_ridge)
        if (it + 1) % check_every:
            continue
        smooth = smooth_losses(P, A, Y).sum() + lam_ridge * (P["w2"] ** 2).sum()
        mean_loss = (smooth + lam * penalty(P)) / p
        losses.append(float(mean_loss))
        if mean_loss < best_loss:
            best_loss, best_it, best = mean_loss, it, {k: v.clone() for k, v in P.items()}
        elif best_it is None:
            raise ValueError("cmlp_ref: the first check's loss is not finite")
        elif it - best_it == lookback * check_every:
            last_it = it
            break
    if best is None:
        raise ValueError("cmlp_ref: no check ran")
    return {"params": to_packed(best), "last_params": to_packed(P), "losses": np.array(losses), "n_checks": len(losses),
            "best_it": best_it, "last_it": last_it}


def group_norms(params, p, lag, hidden):
    """|W1_i[:, j, :]| as a p x p float64 matrix, from packed parameters."""
    W1 = from_packed(params, p, lag, hidden, torch.float64)["W1"] if not isinstance(params, dict) else params["W1"].double()
    return torch.sqrt((W1 ** 2).sum(dim=(1, 3))).numpy()


def gc(params, p, lag, hidden):
    """``cMLP.GC()`` as ``cmlp()`` returns it: int p x p, 1 where the group norm is positive."""
    return (group_norms(params, p, lag, hidden) > 0).astype(int)

"""``cmlp`` — mirror of ``RCAEval/graph_construction/cmlp.py:591-618`` on the MI355X engine.

The reference builds ``cMLP(p, lag=5, hidden=[100])`` — per series i one network
``Conv1d(p, 100, 5)`` -> ReLU -> ``Conv1d(100, 1, 1)`` predicting ``X[t + lag, i]`` from
``X[t .. t + lag - 1, :]`` — and trains all of them with ``train_model_ista`` (``:478-540``):
full-batch gradient steps on ``sum_i mse_i + lam_ridge * sum_i |w2_i|^2`` followed by the
hierarchical group-lasso prox on the first layer (``prox_update``, penalty "H"), with an
early-stopping check every ``check_every`` iterations that keeps the best model. The result is
the int matrix ``adj[i, j] = 1`` iff the first-layer weights of network i on series j are not all
zero (``cMLP.GC``). The whole loop is one engine call (``pcg_cmlp_train``, ``csrc/cmlp.hip``).

Packed parameters: one fp32 vector, the networks in order, per network ``W1[hidden][p][lag]``,
``b1[hidden]``, ``w2[hidden]``, ``b2[1]`` — the layouts of ``Conv1d.weight`` / ``.bias``, so a
``state_dict`` copies straight in (``pack_state_dict``).

Starting point: the reference starts from torch's default ``Conv1d`` initialisation, unseeded.
``default_init`` builds the same layers on the CPU in the same order (per network
``nn.Conv1d(p, hidden, lag)`` then ``nn.Conv1d(hidden, 1, 1)``), so under ``torch.manual_seed`` it
returns the tensors ``cMLP(p, lag, [hidden])`` would hold; ``init=`` takes a packed array instead.

The call raises ``ValueError`` — through ``@rca`` the method then returns the dummy ranking —
where the reference raises: the first check's loss is NaN or Inf (``it - best_it`` with
``best_it = None``), no check ever runs (``max_iter < check_every``: ``restore_parameters(None)``),
or ``T <= lag`` (no sample: the convolution refuses the input).
"""
from __future__ import annotations

import numpy as np


def limits() -> dict:
    """The limits the library's cMLP kernels were built with (``pcg_cmlp_limits``)."""
    import ctypes
    from .. import _lib
    v = [ctypes.c_int32() for _ in range(3)]
    _lib.load().pcg_cmlp_limits(*(ctypes.byref(x) for x in v))
    return {"max_hidden": v[0].value, "max_lag": v[1].value, "max_p": v[2].value}


def network_size(p: int, lag: int, hidden: int) -> int:
    """Floats per network in the packed layout."""
    return hidden * p * lag + 2 * hidden + 1


def pack(networks) -> np.ndarray:
    """Packed fp32 vector from per-network ``(W1, b1, w2, b2)`` arrays (``w2`` of any shape with
    ``hidden`` elements, e.g. the second ``Conv1d``'s ``(1, hidden, 1)`` weight)."""
    parts = []
    for W1, b1, w2, b2 in networks:
        parts += [np.asarray(a, dtype=np.float32).reshape(-1) for a in (W1, b1, w2, b2)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def unpack(params, p: int, lag: int, hidden: int) -> list:
    """Per-network ``(W1[hidden, p, lag], b1[hidden], w2[hidden], b2[1])`` views of a packed vector."""
    params = np.asarray(params).reshape(-1)
    size = network_size(p, lag, hidden)
    if params.size != p * size:
        raise ValueError(f"cmlp: packed parameters hold {params.size} floats, p={p} lag={lag} hidden={hidden} "
                         f"needs {p * size}")
    out, nw = [], hidden * p * lag
    for i in range(p):
        v = params[i * size:(i + 1) * size]
        out.append((v[:nw].reshape(hidden, p, lag), v[nw:nw + hidden], v[nw + hidden:nw + 2 * hidden],
                    v[nw + 2 * hidden:]))
    return out


def pack_state_dict(state_dict, p: int) -> np.ndarray:
    """Packed vector from the ``state_dict`` of the reference's ``cMLP`` (keys
    ``networks.{i}.layers.{0,1}.{weight,bias}``)."""
    def get(i, layer, what):
        t = state_dict[f"networks.{i}.layers.{layer}.{what}"]
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return pack([(get(i, 0, "weight"), get(i, 0, "bias"), get(i, 1, "weight"), get(i, 1, "bias")) for i in range(p)])


def default_init(p: int, lag: int = 5, hidden: int = 100) -> np.ndarray:
    """torch's default initialisation of ``cMLP(p, lag, [hidden])``, packed: the same layers built
    on the CPU in the same order, so the global RNG is consumed exactly as the reference does."""
    import torch.nn as nn
    nets = []
    for _ in range(p):
        l0 = nn.Conv1d(p, hidden, lag)
        l1 = nn.Conv1d(hidden, 1, 1)
        nets.append(tuple(t.detach().numpy() for t in (l0.weight, l0.bias, l1.weight, l1.bias)))
    return pack(nets)


def gc_from_params(params, p: int, lag: int, hidden: int) -> np.ndarray:
    """``cMLP.GC()`` as ``cmlp()`` returns it: int ``adj[i, j] = 1`` iff ``|W1_i[:, j, :]| > 0``."""
    adj = np.zeros((p, p), dtype=int)
    for i, (W1, _b1, _w2, _b2) in enumerate(unpack(params, p, lag, hidden)):
        adj[i] = (np.abs(W1).max(axis=(0, 2)) > 0).astype(int)
    return adj


def cmlp(data, max_iter=None, *, lam=0.002, lam_ridge=1e-2, lr=5e-2, lag=5, hidden=100, check_every=1000,
         lookback=5, init=None, return_info=False):
    """``cmlp.py:591-618``: p x p int matrix, ``adj[i, j] = 1`` iff series j Granger-causes series
    i in the trained cMLP. ``data``: a frame or a T x p array (NaNs forward-filled as the reference
    does). ``init``: packed starting parameters (default ``default_init``). ``return_info``: also
    the engine's dict (``params`` as a host array, ``losses``, ``n_checks``, ``best_it``,
    ``last_it``)."""
    import pandas as pd
    if max_iter is None:
        max_iter = 50000
    frame = data if isinstance(data, pd.DataFrame) else pd.DataFrame(np.asarray(data))
    X = frame.ffill().to_numpy().astype(float).astype(np.float32)
    if X.ndim != 2:
        raise ValueError("cmlp: data must be T x p")
    T, p = X.shape
    lag, hidden = int(lag), int(hidden)
    if T <= lag:
        raise ValueError(f"cmlp: no sample to fit (T={T} <= lag={lag})")
    if max_iter < check_every:
        raise ValueError(f"cmlp: no check runs (max_iter={max_iter} < check_every={check_every})")
    lim = limits()
    if not (1 <= hidden <= lim["max_hidden"] and 1 <= lag <= lim["max_lag"] and 1 <= p <= lim["max_p"]):
        from .._lib import PCG_ERR_INVALID, PcgError
        raise PcgError(PCG_ERR_INVALID, f"cmlp: hidden={hidden}, lag={lag}, p={p} outside the kernels' limits {lim}")
    params = default_init(p, lag, hidden) if init is None else np.asarray(init, dtype=np.float32).reshape(-1)
    from ..engine import get_engine
    out = get_engine().cmlp_train(X, params, max_iter=int(max_iter), lag=lag, hidden=hidden, lr=lr, lam=lam,
                                  lam_ridge=lam_ridge, check_every=int(check_every), lookback=int(lookback))
    out["params"] = out["params"].cpu().numpy()
    adj = gc_from_params(out["params"], p, lag, hidden)
    return (adj, out) if return_info else adj


__all__ = ["cmlp", "default_init", "gc_from_params", "limits", "network_size", "pack", "pack_state_dict", "unpack"]

"""CPU: the cMLP restatement (tests/cmlp_ref.py) against the reference's own recorded answers
(tests/golden/cmlp.npz / cmlp.json, made by tests/golden/make_cmlp_golden.py), the packed
parameter layout, the init helper, the registry entries and the errors that need no device.

Tolerances come from the golden alone. D of a run is the largest absolute parameter difference
between the reference's fp32 runs (1 and 4 torch threads) and its fp64 run; the restatement in fp32
is one more fp32 ordering of the same trajectory and must stay within 4 D of the reference's fp32
parameters. A check loss must stay within 4 max(loss_D, 2^-23 loss) of the recorded one: loss_D is
the same spread measured on the losses, and 2^-23 loss is the spacing of the fp32 number the
reference stores the loss in.
"""
import json
import os

import numpy as np
import pytest
import torch

import cmlp_ref as cr
from rcaeval_amd.graph_construction import cmlp as cm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "cmlp.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN, "cmlp.npz")))


def _kw(m):
    return {k: m[k] for k in ("lam", "lr", "lam_ridge", "max_iter", "check_every", "lookback")}


@pytest.mark.parametrize("k", [1, 25, 400])
def test_restatement_steps_match_the_reference(golden, k):
    meta, g = golden
    s = meta["steps"]
    D = s["D"][str(k)]
    X = cr.var5()
    for dtype, key, tol in ((torch.float32, "f32", 4 * D), (torch.float64, "f64", 4 * D)):
        got, _ = cr.steps(X, g["init"], k, lr=s["lr"], lam=s["lam"], lam_ridge=s["lam_ridge"], dtype=dtype)
        err = np.abs(got - g[f"steps{k}_{key}"].astype(np.float64)).max()
        print(f"k={k} {key}: restatement vs reference {err:.3e}, 4 D = {tol:.3e}")
        assert err <= tol


@pytest.mark.parametrize("name", ["sparse", "early"])
@pytest.mark.parametrize("key,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_restatement_training_matches_the_reference(golden, name, key, dtype):
    meta, g = golden
    m = meta[name]
    out = cr.train(cr.var5(), g["init"], dtype=dtype, **_kw(m))
    assert (out["n_checks"], out["best_it"], out["last_it"]) == (m["n_checks"], m["best_it"], m["last_it"])
    ref_losses = g[f"{name}_losses_{key}"]
    tol = 4 * np.maximum(m["loss_D"], 2.0 ** -23 * np.abs(ref_losses))
    assert (np.abs(out["losses"] - ref_losses) <= tol).all()
    np.testing.assert_array_equal(cr.gc(out["params"], 5, 5, 100), g[f"{name}_gc_{key}"])
    assert np.abs(out["params"] - g[f"{name}_{key}"].astype(np.float64)).max() <= 4 * m["D"]


def test_golden_preconditions(golden):
    meta, g = golden
    for name in ("sparse", "early"):
        m = meta[name]
        assert m["gc_equal"] and m["n_checks"] == m["n_checks_f32"]
        np.testing.assert_array_equal(g[f"{name}_gc_f32"], g[f"{name}_gc_f64"])
    assert (meta["early"]["n_checks"], meta["early"]["best_check"], meta["early"]["last_it"]) == (9, 5, 89)
    gc = g["sparse_gc_f64"]
    assert gc.diagonal().all() and gc[1, 0] and gc[2, 1] and gc[4, 3]


def test_registry_and_exports():
    import rcaeval_amd.e2e as e2e
    from rcaeval_amd import rq2
    assert "cmlp_pagerank" in e2e.__all__ and callable(e2e.cmlp_pagerank)
    assert rq2.methods()["cmlp_pagerank"] is e2e.cmlp_pagerank
    assert set(cm.__all__) >= {"cmlp", "default_init", "pack", "unpack", "pack_state_dict", "gc_from_params"}


def _torch_model(p, lag, hidden):
    """The reference model's module tree (names as in its state_dict), built here."""
    import torch.nn as nn
    nets = nn.ModuleList()
    for _ in range(p):
        net = nn.Module()
        net.layers = nn.ModuleList([nn.Conv1d(p, hidden, lag), nn.Conv1d(hidden, 1, 1)])
        nets.append(net)
    model = nn.Module()
    model.networks = nets
    return model


def test_packed_layout_round_trip():
    p, lag, hidden = 3, 4, 7
    torch.manual_seed(5)
    sd = _torch_model(p, lag, hidden).state_dict()
    packed = cm.pack_state_dict(sd, p)
    assert packed.dtype == np.float32 and packed.size == p * cm.network_size(p, lag, hidden)
    for i, (W1, b1, w2, b2) in enumerate(cm.unpack(packed, p, lag, hidden)):
        np.testing.assert_array_equal(W1, sd[f"networks.{i}.layers.0.weight"].numpy())
        np.testing.assert_array_equal(b1, sd[f"networks.{i}.layers.0.bias"].numpy())
        np.testing.assert_array_equal(w2, sd[f"networks.{i}.layers.1.weight"].numpy().reshape(-1))
        np.testing.assert_array_equal(b2, sd[f"networks.{i}.layers.1.bias"].numpy())
    np.testing.assert_array_equal(cm.pack(cm.unpack(packed, p, lag, hidden)), packed)
    # the restatement reads the same layout
    P = cr.from_packed(packed, p, lag, hidden, torch.float32)
    np.testing.assert_array_equal(P["W1"][1].numpy(), sd["networks.1.layers.0.weight"].numpy())
    np.testing.assert_array_equal(cr.to_packed(P).astype(np.float32), packed)
    with pytest.raises(ValueError):
        cm.unpack(packed[:-1], p, lag, hidden)


def test_default_init_consumes_the_rng_like_the_reference_model(golden):
    _meta, g = golden
    torch.manual_seed(0)
    np.testing.assert_array_equal(cm.default_init(5, 5, 100), g["init"])      # the reference's cMLP(5, 5, [100])
    torch.manual_seed(11)
    a = cm.default_init(3, 2, 6)
    torch.manual_seed(11)
    np.testing.assert_array_equal(a, cm.pack_state_dict(_torch_model(3, 2, 6).state_dict(), 3))


def test_gc_from_params():
    p, lag, hidden = 3, 2, 4
    packed = cr.random_params(p, lag, hidden, seed=1)
    nets = cm.unpack(packed, p, lag, hidden)
    nets[0][0][:, 1, :] = 0.0
    nets[2][0][:, 0, :] = 0.0
    nets[2][0][0, 0, 1] = 1e-30
    want = np.ones((p, p), dtype=int)
    want[0, 1] = 0
    np.testing.assert_array_equal(cm.gc_from_params(packed, p, lag, hidden), want)
    np.testing.assert_array_equal(cr.gc(packed, p, lag, hidden), want)


def test_errors_that_need_no_device():
    X = cr.var5()
    with pytest.raises(ValueError, match="no sample"):
        cm.cmlp(X[:5])
    with pytest.raises(ValueError, match="no check"):
        cm.cmlp(X, max_iter=999)
    with pytest.raises(ValueError, match="no check"):
        cm.cmlp(X, max_iter=10, check_every=11)
    with pytest.raises(ValueError):
        cr.train(X[:5], cr.random_params(5, 5, 4, 0), 10, hidden=4, check_every=5)
    with pytest.raises(ValueError):
        cr.train(X, cr.random_params(5, 5, 4, 0), 4, hidden=4, check_every=5)

"""IRGAN on the device (csrc/irgan.h through aaerec/irgan.py and _hip.irgan_*): the fixtures of the real reference replayed with
their recorded draws, D and G steps against the float64 host route on random states, the device sampler against its
restatement, scores and ranking, determinism, and Evaluation's ranking branch end to end.  tests/irgan_cases.py states the
tolerances and the shapes: item counts one below, at and one above the kernels' tile of 128 rows and one of four tiles; two
user tiles throughout."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import irgan_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
USERS = IC.TILE + 2           # two tiles of user rows, the second nearly empty


def _device_net(net):
    from aaerec import _hip
    return _hip.DeviceIrganNet(net, DEV)


def _up(a, dt):
    from aaerec import _hip
    return _hip.upload(np.ascontiguousarray(a, dtype=dt), DEV)


def _bound(h32, h64):
    """4 x the float32 host route's own distance from the float64 one, floored at 1e-6."""
    from aaerec.irgan import KEYS
    return max(4 * max(float(np.abs(h32[k].astype(np.float64) - h64[k]).max()) for k in KEYS), 1e-6)


def _hold(got, h64, tol, what):
    from aaerec.irgan import KEYS
    worst = 0.0
    for k in KEYS:
        d = float(np.abs(got[k].astype(np.float64) - h64[k]).max())
        worst = max(worst, d)
        assert d <= tol, "{}: {} differs from the float64 host route by {:.3g} (bound {:.3g})".format(what, k, d, tol)
    return worst


# ---- 5. the reference's fixtures on the device -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IC.FIXTURES)
def test_fixture_replay_on_the_device(name):
    fx = IC.Fixture(name)
    model, states, losses = fx.replay(device=DEV)
    assert model.route() == "device" and len(states) == fx.cfg["n_blocks"]
    worst = IC.compare_states(fx, states, IC.TOL_PARAM, name + " device")
    print(name, "device: largest parameter / momentum difference from the reference", worst)
    np.testing.assert_allclose(losses, fx.block_losses(), rtol=IC.TOL_LOSS_R, atol=IC.TOL_LOSS_A)
    pred = model.predict({u: None for u in range(fx.cfg["users"])})
    np.testing.assert_allclose(pred, fx.z["pred"], atol=IC.TOL_PARAM, rtol=0)
    for u, items in fx.X.items():
        assert (pred[u, items] == 0).all()


# ---- 6. D steps ----------------------------------------------------------------------------------------------------------------
def _d_scenarios(rng, users, items):
    one = rng.randint(0, [users, items, items], size=(3, 3))                          # batches of 1 line, 3 steps
    u, i = rng.randint(users), rng.randint(items)
    same = np.tile([[u, i, i]], (20, 1))                                              # every line the same user and item: 8, 8, 4
    mixed = rng.randint(0, [users, items, items], size=(35, 3))                       # 16, 16 and a last short batch of 3
    mixed[5:9, 0] = mixed[4, 0]
    mixed[10:14, 1] = mixed[9, 2]                                                     # repeated users, an item on both sides
    return [("one line", one, 1), ("same user and item", same, 8), ("mixed", mixed, 16)]


@pytest.mark.parametrize("items", IC.ITEM_COUNTS)
@pytest.mark.parametrize("dim", IC.DIMS)
def test_d_steps_against_the_float64_host_route(dim, items):
    from aaerec import _hip, irgan as I
    rng = np.random.RandomState(dim * 1000 + items)
    lr, lam = 0.05, 0.1 / 16
    for what, lines, batch in _d_scenarios(rng, USERS, items):
        net = IC.random_net(rng, USERS, items, dim)
        h32, h64 = I.cast_net(net, np.float32), I.cast_net(net, np.float64)
        l32 = I.host_d_steps(h32, lines, batch, lr, I.MOMENTUM, lam)
        l64 = I.host_d_steps(h64, lines, batch, lr, I.MOMENTUM, lam)
        assert len(l64) == 3
        dn = _device_net(net)
        out = _hip.irgan_d_steps(dn, _up(lines, np.int32), batch, 3, lr, I.MOMENTUM, lam, _hip.irgan_scratch(dn), losses=True)
        tol = _bound(h32, h64)
        worst = _hold(dn.arrays(), h64, tol, "D {} dim {} items {}".format(what, dim, items))
        ltol = max(4 * float(np.abs(np.asarray(l32) - l64).max()), 1e-6)
        print("D", what, dim, items, "device - float64 host:", worst, "bound", tol, "loss", float(np.abs(out.cpu().numpy() - l64).max()), ltol)
        np.testing.assert_allclose(out.cpu().numpy(), l64, atol=ltol, rtol=0)


# ---- 7. G steps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("items", IC.ITEM_COUNTS)
@pytest.mark.parametrize("dim", IC.DIMS)
def test_g_steps_with_injected_samples_against_the_float64_host_route(dim, items):
    from aaerec import _hip, irgan as I
    rng = np.random.RandomState(7 + dim * 1000 + items)
    G, D = IC.random_net(rng, USERS, items, dim), IC.random_net(rng, USERS, items, dim)
    rare = items - 2
    G["item_bias"][rare] = -40.0                       # p under 1e-8: the clamp
    a, b = 3, IC.TILE + 1                              # two users, one in each tile of user rows
    pos = {a: np.asarray([items - 1]), b: np.sort(rng.choice(items - 2, size=6, replace=False))}
    steps = [(a, np.asarray([5, 5])),                                                   # one positive; both samples hit one item
             (b, np.concatenate([rng.randint(0, items, size=9), [rare], pos[b][:2]])),  # repeats, the clamped item, two positives
             (a, np.asarray([items - 1, rare]))]                                        # the first user again: its positive, the clamp
    lr = 0.05
    h = {dt: (I.cast_net(G, dt), I.cast_net(D, dt)) for dt in (np.float32, np.float64)}
    hl = {dt: [I.host_g_step(h[dt][0], h[dt][1], u, pos[u], s, lr, I.MOMENTUM) for u, s in steps] for dt in h}
    g, d = _device_net(G), _device_net(D)
    counts = np.zeros(USERS, dtype=np.int64)
    for u, p in pos.items():
        counts[u] = p.size
    pos_dev = (_up(np.concatenate(([0], np.cumsum(counts))), np.int64), _up(np.concatenate([pos[u] for u in sorted(pos)]), np.int32))
    samples = _up(np.concatenate([s for _, s in steps]), np.int32)
    off = _up(np.concatenate(([0], np.cumsum([s.size for _, s in steps]))), np.int64)
    out = _hip.irgan_g_steps(g, d, _up([u for u, _ in steps], np.int32), pos_dev, 6, lr, I.MOMENTUM, _hip.irgan_scratch(g),
                             samples=samples, sample_off=off, losses=True)
    tol = _bound(h[np.float32][0], h[np.float64][0])
    got = g.arrays()
    worst = _hold(got, h[np.float64][0], tol, "G dim {} items {}".format(dim, items))
    ltol = max(4 * float(np.abs(np.asarray(hl[np.float32]) - hl[np.float64]).max()), 1e-6)
    print("G", dim, items, "device - float64 host:", worst, "bound", tol, "loss", float(np.abs(out.cpu().numpy() - hl[np.float64]).max()), ltol)
    np.testing.assert_allclose(out.cpu().numpy(), hl[np.float64], atol=ltol, rtol=0)
    # the dense momentum carry: a user row no step names has moved, by the momentum alone
    idle = 0
    want = G["user_emb"][idle].astype(np.float64) - lr * G["m_user_emb"][idle] * (0.9 + 0.81 + 0.729)
    assert (got["user_emb"][idle] != G["user_emb"][idle]).any()
    np.testing.assert_allclose(got["user_emb"][idle], want, atol=1e-6, rtol=0)
    for k in I.KEYS:                                    # D is read, never written
        assert (d.arrays()[k] == D[k]).all()


# ---- 8. the device sampler ---------------------------------------------------------------------------------------------------------
def _sampler_setup(name):
    from aaerec import _hip
    net, pos = IC.sampler_case(name)
    users = sorted(pos)
    n = [pos[u].size for u in users]
    off = np.concatenate(([0], np.cumsum(n))).astype(np.int64)
    lines = np.zeros((off[-1], 3), dtype=np.int32)
    for q, u in enumerate(users):
        lines[off[q]:off[q + 1], 0] = u
        lines[off[q]:off[q + 1], 1] = pos[u]
        lines[off[q]:off[q + 1], 2] = -7
    dn = _device_net(net)
    return net, pos, users, off, lines, dn, _hip.irgan_scratch(dn, slots=5)


def _agree(got, want, flags, what):
    off_boundary = (got != want) & ~flags
    assert not off_boundary.any(), "{}: {} draws differ away from a boundary".format(what, int(off_boundary.sum()))
    excused = int((got != want).sum())
    print(what, "flagged", int(flags.sum()), "differing", excused, "of", got.size)
    assert flags.sum() <= 0.01 * got.size


@pytest.mark.parametrize("name", sorted(IC.SAMPLER_CASES))
def test_device_sampler_equals_its_restatement(name):
    from aaerec import _hip, irgan as I
    seed, draw = 77, 3
    net, pos, users, off, lines, dn, scratch = _sampler_setup(name)
    neg, smp = IC.restated_draws(name, seed, draw)
    max_pos = int(np.diff(off).max())

    def negatives(chunks, draw):
        ld = _up(lines, np.int32)
        for lo, hi in chunks:
            _hip.irgan_sample_neg(dn, _up(users[lo:hi], np.int32), _up(off[lo:hi + 1], np.int64), max_pos, I.TEMPERATURE, seed, draw, ld, scratch)
        got = ld.cpu().numpy()
        assert (got[:, :2] == lines[:, :2]).all() and got[:, 2].min() >= 0 and got[:, 2].max() < dn.items
        return got[:, 2]

    n = len(users)
    whole = negatives([(0, n)], draw)
    _agree(whole, np.concatenate([neg[u][0] for u in users]), np.concatenate([neg[u][1] for u in users]), name + " negatives")
    assert (negatives([(q, q + 1) for q in range(n)], draw) == whole).all()              # users chunked 1 / 3 / all: the same lines
    assert (negatives([(q, min(q + 3, n)) for q in range(0, n, 3)], draw) == whole).all()
    assert (negatives([(0, n)], draw + 1) != whole).any()                                # another draw counter: other lines
    # the G-step draws: lr = 0 leaves every logit where it is, so every user draws from the parameters of the case
    D = _device_net(IC.random_net(np.random.RandomState(5), dn.users, dn.items, dn.dim))
    counts = np.zeros(dn.users, dtype=np.int64)
    counts[users] = [pos[u].size for u in users]
    pos_dev = (_up(np.concatenate(([0], np.cumsum(counts))), np.int64), _up(np.concatenate([pos[u] for u in users]), np.int32))
    soff = np.concatenate(([0], np.cumsum([2 * pos[u].size for u in users]))).astype(np.int64)
    out = torch.full((int(soff[-1]),), -7, dtype=torch.int32, device=DEV)
    _hip.irgan_g_steps(dn, D, _up(users, np.int32), pos_dev, max_pos, 0.0, I.MOMENTUM, scratch, sample_off=_up(soff, np.int64),
                       seed=seed, draw=draw, samples_out=out)
    _agree(out.cpu().numpy(), np.concatenate([smp[u][0] for u in users]), np.concatenate([smp[u][1] for u in users]), name + " samples")
    assert (dn.arrays()["item_emb"] == net["item_emb"]).all()


# ---- 9. scores and ranking ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranked():
    """A model of 40 users over 385 items with negative and positive ratings, user 5 without training positives; the test rows:
    row 0 knows every item, row 1 none, the rest a few."""
    from aaerec import irgan as I
    rng = np.random.RandomState(21)
    users, items, dim = 40, 3 * IC.TILE + 1, 5
    net = IC.random_net(rng, users, items, dim)
    X = {u: rng.choice(items, size=rng.randint(1, 12), replace=False).tolist() for u in range(users) if u != 5}
    m = I.IRGAN(users, items, emb_dim=dim, verbose=False, device=DEV, seed=1, scratch_bytes=4 * (items + 3) * 7)      # 7 rows a chunk
    state = {pre + k: net[k] for pre in ("gen.", "dis.") for k in I.KEYS}
    lists = list(X.values())
    state.update(train_users=np.asarray(list(X)), train_indptr=np.concatenate(([0], np.cumsum([len(v) for v in lists]))),
                 train_items=np.concatenate(lists))
    m.load_state_dict(state)
    rows = np.arange(30)
    known = sp.lil_matrix((rows.size, items))
    known[0, :] = 1
    for r in range(2, rows.size):
        known[r, rng.choice(items, size=rng.randint(1, 9), replace=False)] = 1
    known = known.tocsr()
    truth = sp.lil_matrix((rows.size, items))
    for r in range(rows.size):
        truth[r, rng.choice(items, size=rng.randint(1, 4), replace=False)] = 1
    truth[2, known[2].indices[0]] = 1                      # a held-out item that is a known item
    return m, net, X, rows, known, truth.tocsr()


def test_scores_hold_the_bound_and_training_positives_are_exactly_zero(ranked):
    """|device - exact| <= 2^-24 (dim + 2) sum |u| |v| per element, the sum over the dim + 1 terms of the chain the kernel runs
    (the bias is its first term, 1 * item_bias[j]): dim fmaf roundings at most, and two units to spare."""
    m, net, X, rows, known, truth = ranked
    got = m.predict({u: None for u in range(m.user_num)})
    U, V, b = (net[k].astype(np.float64) for k in ("user_emb", "item_emb", "item_bias"))
    exact = U @ V.T + b
    bound = 2.0 ** -24 * (m.emb_dim + 2) * (np.abs(U) @ np.abs(V).T + np.abs(b))
    mask = np.zeros(exact.shape, dtype=bool)
    for u, it in X.items():
        mask[u, it] = True
    assert (got[mask] == 0).all() and not mask[5].any() and (got[5] != 0).all()
    err = np.abs(got - exact)[~mask]
    print("scores: largest error / bound", float((err / bound[~mask]).max()))
    assert (err <= bound[~mask]).all()


def test_lists_and_ranks_are_the_host_rankers_on_the_devices_own_scores(ranked):
    from aaerec import ranking
    from aaerec.irgan import _scaled
    m, net, X, rows, known, truth = ranked
    scores = m.predict({int(u): None for u in rows})
    host_rows = lambda: ranking.host_rows(known, lambda r0, r1: scores[r0:r1])      # noqa: E731
    assert m.route() == "device" and m._chunk_rows(m.item_num) == 7
    for k in (1, 10, m.item_num):
        ids, val = m.predict_topk(rows, known, k=k)
        want_ids, want_val = ranking.host_topk(host_rows(), rows.size, k, _scaled)
        assert ids.dtype == np.int32 and (ids == want_ids).all(), k
        np.testing.assert_allclose(val, want_val, atol=2e-6, rtol=0)
    ids, _ = m.predict_topk(rows, known, k=m.item_num)
    assert (ids[0] == -1).all()                                # a row whose every item is known
    assert (ids[1] >= 0).all() and sorted(ids[1]) == list(range(m.item_num))
    # the reference's quirk, pinned on purpose: a training positive is a 0, and outranks every negative rating
    r = 3
    zero_at = [int(np.nonzero(ids[r] == i)[0][0]) for i in X[r] if i not in known[r].indices]
    negatives = np.nonzero(scores[r] < 0)[0]
    assert zero_at and negatives.size > 50
    assert max(zero_at) < min(int(np.nonzero(ids[r] == j)[0][0]) for j in negatives if j not in known[r].indices)
    ranks = m.predict_ranks(rows, known, truth)
    want = ranking.host_ranks(host_rows(), ranking.canonical_truth(truth, known.shape))
    assert ranks.dtype == np.int32 and (ranks.indptr == want.indptr).all() and (ranks.data == want.data).all()
    assert ranks.data.min() >= 1


# ---- 10. determinism -----------------------------------------------------------------------------------------------------------
def test_two_fits_with_one_seed_are_bit_identical():
    from aaerec.irgan import IRGAN, KEYS
    fx = IC.Fixture("irgan_small")
    c = fx.cfg
    runs = []
    for seed in (3, 3, 4):
        m = IRGAN(c["users"], c["items"], batch_size=c["batch_size"], lr=c["lr"], n_epochs=2, d_epochs=6, g_epochs=2, verbose=False,
                  device=DEV, seed=seed)
        assert m.route() == "device"
        runs.append(m.fit(fx.X).state_dict())
    for net in ("gen.", "dis."):
        for k in KEYS:
            assert (runs[0][net + k] == runs[1][net + k]).all(), net + k
    assert any((runs[0]["gen." + k] != runs[2]["gen." + k]).any() for k in KEYS)
    assert np.isfinite(runs[0]["gen.item_emb"]).all() and (runs[0]["dis.m_item_emb"] != 0).any()


# ---- 11. end to end ------------------------------------------------------------------------------------------------------------
def _toy_bags():
    from aaerec.datasets import Bags
    rng = np.random.RandomState(0)
    protos = [rng.choice(40, size=8, replace=False) for _ in range(6)]
    data, owners, years = [], [], {}
    for i in range(60):
        data.append(["i%d" % t for t in rng.choice(protos[rng.randint(6)], size=rng.randint(3, 7), replace=False)])
        owners.append("d%d" % i)
        years["d%d" % i] = 2000 + (i * 10) // 60
    return Bags(data, owners, {"year": years})


def test_evaluation_ranks_the_recommender_on_the_device():
    from aaerec import ranking
    from aaerec.evaluation import Evaluation, evaluate_ranks, evaluate_topk
    from aaerec.irgan import IRGANRecommender, _scaled
    bags = _toy_bags()
    for metrics, method in ((["mrr@10", "map@10", "p@5", "P@1"], "predict_topk"), (["mrr", "map", "mrr@10"], "predict_ranks")):
        ev = Evaluation(bags, 2008, metrics=metrics, logfile=None, topk=True).setup(min_elements=2, drop=1)
        user_num = ev.train_set.size()[0] + ev.test_set.size()[0]
        rec = IRGANRecommender(user_num, ev.train_set.size()[1], n_epochs=1, d_epochs=1, g_epochs=1, lr=0.05, verbose=False, seed=5)
        calls = []
        real = getattr(rec, method)
        setattr(rec, method, lambda *a, _real=real, **kw: calls.append(1) or _real(*a, **kw))
        res = ev([rec])[0]
        assert len(calls) == 1 and rec.route() == "device"
        pred = np.asarray(rec.predict(ev.test_set))            # the same trained model's dense scores, ranked by the host
        X = sp.csr_matrix(ev.x_test)
        X.sum_duplicates()
        X.sort_indices()
        rows = lambda: ranking.host_rows(X, lambda r0, r1: pred[r0:r1])      # noqa: E731
        if method == "predict_topk":
            want = evaluate_topk(ev.y_test, ranking.host_topk(rows(), X.shape[0], 10, _scaled)[0], metrics)
        else:
            want = evaluate_ranks(ranking.host_ranks(rows(), ranking.canonical_truth(ev.y_test, X.shape)), metrics)
        print(method, np.asarray(res).ravel().tolist())
        np.testing.assert_allclose(np.asarray(res), np.asarray(want), atol=0, rtol=0)

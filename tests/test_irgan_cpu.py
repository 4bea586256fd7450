"""What IRGAN (aaerec/irgan.py, csrc/irgan.h, csrc/abi_irgan.h) needs no device for: the host route against the fixtures recorded
from the real reference, the sampler restatement's distribution and its boundary sensitivity, the library's surface and its
argument checks, the routes and the refusals (tests/irgan_cases.py states the tolerances)."""
import ctypes as C

import numpy as np
import pytest

import irgan_cases as IC


# ---- 1. the host route against the reference ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replays():
    out = {}
    for name in IC.FIXTURES:
        fx = IC.Fixture(name)
        out[name] = (fx, {dt: fx.replay(device=None, host_dtype=dt) for dt in (np.float32, np.float64)})
    return out


@pytest.mark.parametrize("name", IC.FIXTURES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_route_replays_the_reference(replays, name, dtype):
    fx, runs = replays[name]
    model, states, losses = runs[dtype]
    assert model.route() is None and len(states) == fx.cfg["n_blocks"]
    worst = IC.compare_states(fx, states, IC.TOL_PARAM, "{} {}".format(name, dtype.__name__))
    print(name, dtype.__name__, "largest parameter / momentum difference from the reference", worst)
    np.testing.assert_allclose(losses, fx.block_losses(), rtol=IC.TOL_LOSS_R, atol=IC.TOL_LOSS_A)
    pred = model.predict({u: None for u in range(fx.cfg["users"])})
    assert pred.shape == fx.z["pred"].shape and pred.dtype == np.float64
    np.testing.assert_allclose(pred, fx.z["pred"], atol=IC.TOL_PARAM, rtol=0)
    for u, items in fx.X.items():
        assert (pred[u, items] == 0).all()                 # the training positives: exactly 0, not -inf


@pytest.mark.parametrize("name", IC.FIXTURES)
def test_the_recorded_float32_run_lies_within_a_quarter_of_the_cap_of_the_float64_restatement(replays, name):
    fx, runs = replays[name]
    worst = IC.compare_states(fx, runs[np.float64][1], IC.TOL_PARAM / 4, name + " float64")
    print(name, "reference (float32) against the float64 restatement:", worst)


def test_fixture_shapes_are_what_the_issue_asks_for():
    small, dup = IC.Fixture("irgan_small"), IC.Fixture("irgan_dup")
    assert (small.cfg["users"], small.cfg["items"], small.cfg["batch_size"]) == (7, 40, 4)
    assert all(1 <= len(v) <= 4 for v in small.X.values())
    assert (dup.cfg["users"], dup.cfg["items"], dup.cfg["batch_size"]) == (5, 9, 16)
    assert all(3 <= len(v) <= 6 for v in dup.X.values())
    lines = dup.z["lines"][:16]                              # one D batch holds repeated users and items
    assert len(set(lines[:, 0])) < 16 and len(set(lines[:, 1:].ravel())) < 32
    assert any(len(set(d.tolist())) < d.size for d in dup.draws)      # and the samples repeat
    for fx in (small, dup):                                  # generate_for_d ran twice per epoch
        assert len(fx.z["line_indptr"]) - 1 == 2 * fx.cfg["n_epochs"]


# ---- 2. the sampler draws from the right distribution ---------------------------------------------------------------------------
P8 = np.asarray([0.4, 0.25, 0.15, 0.1, 0.05, 0.025, 0.015, 0.01])
N_DRAWS = 1 << 16


def _within(counts, p, n):
    dev = np.abs(counts - n * p)
    cap = 5 * np.sqrt(n * p * (1 - p))
    assert (dev <= cap).all(), (counts, n * p, cap)


def test_temperature_form_draws_from_the_softmax():
    from aaerec import irgan as I
    logits = (np.log(P8) * I.TEMPERATURE).astype(np.float32)          # logits / temperature = log p
    items = I.draw_negatives(123, 0, 3, N_DRAWS, logits)
    _within(np.bincount(items, minlength=8), P8, N_DRAWS)


def test_mixture_form_draws_from_pn_with_a_positive_among_the_rare_items():
    from aaerec import irgan as I
    pos = np.repeat([6, 7], N_DRAWS // 4)                             # 2 |pos| = 2^16 samples, the positives two rare items
    items = I.draw_samples(123, 1, 3, pos, np.log(P8).astype(np.float32))
    pn = 0.8 * P8
    pn[[6, 7]] += 0.1
    assert items.size == N_DRAWS
    _within(np.bincount(items, minlength=8), pn, N_DRAWS)


def test_a_seed_a_draw_counter_and_a_user_key_the_draws():
    from aaerec import irgan as I
    lg = np.log(P8).astype(np.float32)
    a = I.draw_negatives(5, 0, 1, 64, lg)
    assert (a == I.draw_negatives(5, 0, 1, 64, lg)).all() and (a[:32] == I.draw_negatives(5, 0, 1, 32, lg)).all()
    for other in (I.draw_negatives(6, 0, 1, 64, lg), I.draw_negatives(5, 1, 1, 64, lg), I.draw_negatives(5, 0, 2, 64, lg)):
        assert (a != other).any()


# ---- 3. boundary sensitivity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.SAMPLER_CASES))
def test_boundary_draws_are_rare(name):
    neg, smp = IC.restated_draws(name, seed=77, draw=3)
    for what, d in (("negatives", neg), ("samples", smp)):
        flags = np.concatenate([f for _, f in d.values()])
        print(name, what, "boundary", int(flags.sum()), "of", flags.size)
        assert flags.sum() <= 0.0025 * flags.size


# ---- 4. the library's surface -------------------------------------------------------------------------------------------------
NAMES = ("aae_irgan_scratch_bytes", "aae_irgan_scores", "aae_irgan_topk", "aae_irgan_ranks", "aae_irgan_d_steps",
         "aae_irgan_sample_neg", "aae_irgan_g_steps")


def test_library_exports_the_irgan_calls_and_the_abi_version_stands():
    from aaerec import _hip
    lib = _hip.load_library()
    for name in NAMES:
        assert getattr(lib, name) is not None and name in _hip._PROTOS, name
    assert lib.aae_abi_version() == 4 and _hip.ABI_VERSION == 4
    with open(IC.ROOT + "/include/aaerec_hip.h") as fh:
        header = fh.read()
    for define, value in (("DIM_MAX", _hip.IRGAN_DIM_MAX), ("POS_MAX", _hip.IRGAN_POS_MAX), ("BATCH_MAX", _hip.IRGAN_BATCH_MAX),
                          ("TILE", _hip.IRGAN_TILE)):
        assert "#define AAE_IRGAN_%s %d" % (define, value) in header
    assert _hip.IRGAN_TILE == IC.TILE


def _args(**over):
    """A well-formed set of arguments over pointers nothing may dereference, some replaced."""
    from aaerec import _hip
    p = 0x1000
    g, d, known, truth = _hip.AaeIrganNet(), _hip.AaeIrganNet(), _hip.AaeBatch(), _hip.AaeBatch()
    for n in (g, d):
        for f, _ in _hip.AaeIrganNet._fields_[:6]:
            setattr(n, f, p)
        n.users, n.items, n.dim = 30, 50, 5
    for b in (known, truth):
        b.indptr_dev = b.indices_dev = b.values_dev = p
        b.n_rows = 4
    a = dict(g=g, d=d, known=known, truth=truth, users=p, rows=4, pos_ip=p, pos_it=p, out=p, ld=52, k=10, idx=p, val=p, ranks=p,
             lines=p, n_lines=40, batch=16, steps=3, scratch=p, bytes=1 << 30, line_off=p, n_users=4, max_pos=8, temp=0.2,
             samples=None, sample_off=None, draw=0)
    a.update(over)
    return a


def _call(lib, which, a):
    ref = lambda s: None if s is None else C.byref(s)      # noqa: E731
    if which == "scratch_bytes":
        return lib.aae_irgan_scratch_bytes(ref(a["g"]), C.byref(C.c_size_t()) if a["out"] else None)
    if which == "scores":
        return lib.aae_irgan_scores(ref(a["g"]), a["users"], a["rows"], a["pos_ip"], a["pos_it"], a["out"], a["ld"], None)
    if which == "topk":
        return lib.aae_irgan_topk(ref(a["g"]), a["users"], a["pos_ip"], a["pos_it"], ref(a["known"]), a["k"], 1, a["out"], a["ld"],
                                  a["idx"], a["val"], None)
    if which == "ranks":
        return lib.aae_irgan_ranks(ref(a["g"]), a["users"], a["pos_ip"], a["pos_it"], ref(a["known"]), ref(a["truth"]), 1, a["out"],
                                   a["ld"], a["ranks"], None)
    if which == "d_steps":
        return lib.aae_irgan_d_steps(ref(a["d"]), a["lines"], a["n_lines"], a["batch"], a["steps"], 0.05, 0.9, 0.01, None, a["scratch"],
                                     a["bytes"], None)
    if which == "sample_neg":
        return lib.aae_irgan_sample_neg(ref(a["g"]), a["users"], a["line_off"], a["n_users"], a["max_pos"], a["temp"], 1, a["draw"],
                                        a["lines"], a["n_lines"], a["scratch"], a["bytes"], None)
    return lib.aae_irgan_g_steps(ref(a["g"]), ref(a["d"]), a["users"], a["steps"], a["pos_ip"], a["pos_it"], a["max_pos"], a["samples"],
                                 a["sample_off"], None, 1, a["draw"], 0.05, 0.9, None, a["scratch"], a["bytes"], None)


def _field(kind, field, value, **over):
    def make():
        a = _args(**over)
        setattr(a[kind], field, value)
        return a
    return make


_BAD = [
    # NULL pointers
    ("scratch_bytes", lambda: _args(g=None), "NULL"), ("scratch_bytes", lambda: _args(out=None), "NULL"),
    ("scores", lambda: _args(g=None), "NULL"), ("scores", _field("g", "item_emb_dev", None), "NULL"),
    ("scores", lambda: _args(users=None), "NULL"), ("scores", lambda: _args(out=None), "NULL"),
    ("scores", lambda: _args(pos_it=None), "both or neither"),
    ("topk", lambda: _args(known=None), "NULL"), ("topk", _field("known", "indices_dev", None), "NULL"),
    ("topk", lambda: _args(idx=None), "NULL"), ("topk", lambda: _args(val=None), "NULL"), ("topk", _field("g", "user_emb_dev", None), "NULL"),
    ("ranks", lambda: _args(truth=None), "NULL"), ("ranks", lambda: _args(ranks=None), "NULL"), ("ranks", lambda: _args(out=None), "NULL"),
    ("d_steps", lambda: _args(d=None), "NULL"), ("d_steps", _field("d", "m_item_bias_dev", None), "momentum"),
    ("d_steps", lambda: _args(lines=None), "NULL"), ("d_steps", lambda: _args(scratch=None), "NULL"),
    ("sample_neg", lambda: _args(line_off=None), "NULL"), ("sample_neg", lambda: _args(lines=None), "NULL"),
    ("sample_neg", lambda: _args(scratch=None), "NULL"),
    ("g_steps", lambda: _args(d=None), "NULL"), ("g_steps", _field("g", "m_user_emb_dev", None), "momentum"),
    ("g_steps", lambda: _args(pos_ip=None), "NULL"), ("g_steps", lambda: _args(samples=0x1000), "both or neither"),
    # dim outside [1, 64]
    ("scores", _field("g", "dim", 0), "[1, 64]"), ("topk", _field("g", "dim", 65), "[1, 64]"), ("ranks", _field("g", "dim", -1), "[1, 64]"),
    ("d_steps", _field("d", "dim", 65), "[1, 64]"), ("sample_neg", _field("g", "dim", 0), "[1, 64]"), ("g_steps", _field("d", "dim", 65), "[1, 64]"),
    ("scratch_bytes", _field("g", "dim", 65), "[1, 64]"), ("scores", _field("g", "items", 0), "positive"),
    # k out of range
    ("topk", lambda: _args(k=0), "k must be"), ("topk", lambda: _args(k=51), "k must be"),
    ("topk", _field("g", "items", 5000, k=1025, ld=5000), "k must be"),
    # bad ld / base
    ("scores", lambda: _args(ld=48), "leading dimension"), ("topk", lambda: _args(ld=50), "leading dimension"),
    ("ranks", lambda: _args(ld=53), "leading dimension"), ("scores", lambda: _args(out=0x1004), "aligned"),
    ("ranks", _field("truth", "n_rows", 3), "rows"), ("scores", lambda: _args(rows=-1), "negative"),
    # a batch over 1024 lines, steps beyond the lines
    ("d_steps", lambda: _args(batch=1025, n_lines=4000), "[1, 1024]"), ("d_steps", lambda: _args(batch=0), "[1, 1024]"),
    ("d_steps", lambda: _args(steps=4), "n_steps"),
    # a user with over 2048 positives
    ("sample_neg", lambda: _args(max_pos=2049), "2048 positives"), ("g_steps", lambda: _args(max_pos=2049), "2048 positives"),
    ("sample_neg", lambda: _args(temp=0.0), "temperature"), ("sample_neg", lambda: _args(draw=-1), "negative"),
    # the scratch
    ("d_steps", lambda: _args(bytes=1024), "aae_irgan_scratch_bytes"), ("g_steps", lambda: _args(scratch=0x1010), "256-byte"),
    ("g_steps", _field("d", "items", 51), "other numbers"),
]


@pytest.mark.parametrize("case", range(len(_BAD)))
def test_invalid_arguments_are_refused_before_the_device(case):
    from aaerec import _hip
    lib = _hip.load_library()
    which, make, word = _BAD[case]
    assert _call(lib, which, make()) == -1                  # AAE_EINVAL
    msg = lib.aae_last_error().decode()
    assert msg.startswith("aae_irgan_" + which) and word in msg, msg


def test_calls_without_rows_or_steps_launch_nothing():
    from aaerec import _hip
    lib = _hip.load_library()
    a = _args(rows=0, steps=0, n_users=0)
    a["known"].n_rows = a["truth"].n_rows = 0
    for which in ("scores", "topk", "ranks", "d_steps", "sample_neg", "g_steps"):
        assert _call(lib, which, a) == 0, which
    n = C.c_size_t()
    assert lib.aae_irgan_scratch_bytes(C.byref(a["g"]), C.byref(n)) == 0 and n.value > 2 * 2048 * 5 * 4


def test_routes_and_refusals(monkeypatch):
    import torch
    from aaerec import _hip, irgan as I
    X = {0: [1, 2], 1: [3]}
    assert I.IRGAN(4, 10, device=None, verbose=False).route() is None
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert I.IRGAN(4, 10, verbose=False).route() == "device"
    assert I.IRGAN(4, 10, emb_dim=64, batch_size=1024, verbose=False).route() == "device"
    assert I.IRGAN(4, 10, emb_dim=65, verbose=False).route() is None
    assert I.IRGAN(4, 10, batch_size=1025, verbose=False).route() is None
    m = I.IRGAN(4, 3000, verbose=False)
    m._set_positives({0: list(range(_hip.IRGAN_POS_MAX))})
    assert m.route() == "device"
    m._set_positives({0: list(range(_hip.IRGAN_POS_MAX + 1))})
    assert m.route() is None
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert I.IRGAN(4, 10, verbose=False).route() is None
    for make in (lambda: I.IRGAN(4, 10, conditions=object()), lambda: I.IRGANRecommender(4, 10, conditions=object())):
        with pytest.raises(NotImplementedError, match="optimiser never sees|conditions"):
            make()
    with pytest.raises(NotImplementedError):
        I.IRGAN(4, 10, device=None, verbose=False).fit(X, y=1)
    with pytest.raises(ValueError):
        I.IRGAN(4, 10, draws="torch")
    a, b = I.IRGAN(4, 10, verbose=False), I.IRGAN(4, 10, device=None, draws="numpy", verbose=False)
    assert isinstance(a.seed, int) and b.seed is None      # draws="device" needs a seed: one is drawn and stored


def test_host_route_with_the_keyed_generator_is_a_function_of_the_seed_and_skips_users_without_positives():
    from aaerec import irgan as I
    X = {0: [1, 2, 2], 1: [], 2: [3], 3: [0, 5, 7]}
    runs = []
    for seed in (9, 9, 10):
        m = I.IRGAN(5, 12, batch_size=4, lr=0.05, n_epochs=1, d_epochs=6, g_epochs=2, verbose=False, device=None, seed=seed)
        runs.append(m.fit(X).state_dict())
    assert all((runs[0][k] == runs[1][k]).all() for k in runs[0] if "." in k)
    assert any((runs[0][k] != runs[2][k]).any() for k in runs[0] if "." in k)
    assert runs[0]["draw"] == 2 + 2                           # two generate_for_d, two G epochs
    m = I.IRGAN(5, 12, verbose=False, device=None, seed=1).load_state_dict(runs[0])
    assert all((m.state_dict()[k] == runs[0][k].astype(np.float32)).all() for k in runs[0] if "." in k)
    pred = m.predict({1: None, 3: None, 4: None})
    assert pred.shape == (3, 12) and (pred[1, [0, 5, 7]] == 0).all() and (pred[0] != 0).all() and (pred[2] != 0).all()


def test_recommender_surface_is_the_references():
    from aaerec.irgan import IRGANRecommender
    rec = IRGANRecommender(8, 20, g_epochs=1, d_epochs=1, n_epochs=1)
    assert str(rec) == "IRGAN\nModel Params: " + str(dict(g_epochs=1, d_epochs=1, n_epochs=1))
    for name in ("train", "predict", "predict_topk", "predict_ranks", "route"):
        assert callable(getattr(rec, name))

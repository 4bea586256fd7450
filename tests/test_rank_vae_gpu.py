"""GPU parity of the VAE's predict -> rank (aae_vae_predict_topk / aae_vae_predict_ranks / aae_vae_decode_*; csrc/abi_rank.h,
the VAE's form: the hidden half - fc1, [fc21; fc22], the reparametrisation, the condition block, fc3 - as one program on
the 4-row chain kernel, then the AAE's ranking passes over fc4).  Reference: vae.py:229-266 behind evaluation.py:183-199,
20-58.  Checked against the CPU oracle (oracle.aae_oracle.OracleVAE, same parameters, CSR, injected eps and constant
condition), against the library's own dense form (aae_vae_predict + the host pipeline) and against itself (chunking, the
full ranks against the k = 1024 lists, the device generator against injected zeros).

TOL is the tolerance tests/test_parity_abi_gpu.py holds aae_vae_predict to against this oracle (TOL_RECON = 1e-5); the
fused-against-dense bound 2e-6 and its rule are those of tests/test_rank_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5          # tests/test_parity_abi_gpu.py TOL_RECON: aae_vae_predict against OracleVAE.predict
NEAR_TIE_CAP = 0.02


def _host_topk(full, known_rows, k, exclude_known):
    """tests/test_rank_gpu.py's rule: min-max scale every row over ALL its scores, drop the row's input items, the k best
    (ties: smaller item id first); fewer than k rankable items: -1 / 0 behind them."""
    n, N = full.shape
    ids = np.full((n, k), -1, dtype=np.int64)
    vals = np.zeros((n, k), dtype=np.float32)
    for b in range(n):
        row = full[b].astype(np.float32)
        lo, hi = row.min(), row.max()
        sc = (row - lo) * (np.float32(1.0) / (hi - lo) if hi > lo else np.float32(1.0))
        rk = row.astype(np.float64)
        n_ok = N
        if exclude_known:
            rk[known_rows[b]] = -np.inf
            n_ok = N - len(known_rows[b])
        order = np.lexsort((np.arange(rk.size), -rk))[:min(k, n_ok)]
        ids[b, :len(order)], vals[b, :len(order)] = order, sc[order]
    return ids, vals


def _scaled(full):
    lo, hi = full.min(1), full.max(1)
    return (full - lo[:, None]) / np.where(hi > lo, hi - lo, 1.0)[:, None]


def _corpus(r, N, n_docs, max_len, long_row=None):
    rows = [np.sort(r.choice(N, size=int(r.integers(1, max_len)), replace=False)) for _ in range(n_docs)]
    if long_row is not None:          # a row that names most of the vocabulary: fewer than k items left to rank
        rows[long_row[0]] = np.sort(r.choice(N, size=long_row[1], replace=False))
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32), np.ones(int(ip[-1]), dtype=np.float32), rows


def vae_params(N, h, c, inc, seed, spread=8.0):
    """nn.Linear-style uniform initialisation of the five Linears under the oracle's names; fc4 scaled by `spread` (nn.Linear
    leaves every sigmoid near 0.5: tests/test_rank_gpu.py::_rank_case spreads the logits the same way)."""
    r = np.random.default_rng(seed)

    def lin(o, i):
        b = 1.0 / np.sqrt(i)
        return r.uniform(-b, b, (o, i)).astype(np.float32), r.uniform(-b, b, o).astype(np.float32)
    p = {}
    for name, (o, i) in (("fc1", (h, N)), ("fc21", (c, h)), ("fc22", (c, h)), ("fc3", (h, c + inc)), ("fc4", (N, h))):
        p[name + ".weight"], p[name + ".bias"] = lin(o, i)
    p["fc4.weight"] *= np.float32(spread)
    return p


def to_hip(p):
    return {"enc.lin1.weight": p["fc1.weight"], "enc.lin1.bias": p["fc1.bias"],
            "enc.lin3.weight": np.vstack([p["fc21.weight"], p["fc22.weight"]]),
            "enc.lin3.bias": np.concatenate([p["fc21.bias"], p["fc22.bias"]]),
            "dec.lin1.weight": p["fc3.weight"], "dec.lin1.bias": p["fc3.bias"],
            "dec.lin3.weight": p["fc4.weight"], "dec.lin3.bias": p["fc4.bias"]}


class Case:
    """A VAE handle and the oracle with the same parameters after `steps` training steps on both (the handle then has
    enc.lin1 rows with deferred Adam steps pending and a deferred optimiser launch in flight), a corpus and its eps / cond."""

    def __init__(self, seed, N, h, c, inc, R, rows, max_len=30, long_row=None, steps=3, with_device=True, rng_mode="inject"):
        from oracle import aae_oracle as O
        r = np.random.default_rng(1000 + seed)
        self.N, self.h, self.c, self.inc, self.R, self.rows = N, h, c, inc, R, rows
        p = vae_params(N, h, c, inc, seed)
        self.ora = O.OracleVAE(p, lr=1e-3, conditions=[O.ConcatConst(inc)] if inc else None)
        self.ip, self.idx, self.val, self.docs = _corpus(r, N, rows, max_len, long_row)
        self.eps = r.standard_normal((rows, c)).astype(np.float32)
        self.cond = (r.standard_normal((rows, inc)) * 0.4).astype(np.float32) if inc else None
        # the training batches: a corpus of their own (short rows: within the handle's per-batch bounds)
        tip, tidx, tval, _ = _corpus(r, N, R * max(steps, 1), max_len)
        self.dev = None
        if with_device:       # (False: the oracle alone, on the CPU - how the seeds of the rank cases were checked)
            from aaerec._hip import HipAAE, DeviceCSR
            self.dev = HipAAE(N, h, c, cond_inc=inc, max_batch=R, max_nnz=R * N, rng_mode=rng_mode, seed=7, dropout=(0.0, 0.0),
                              gen_lr=1e-3, reg_lr=1e-3, vae=True)
            self.dev.load_params(to_hip(p))
            self.csr = DeviceCSR.from_arrays(self.ip, self.idx, self.val, N, self.dev.device)
            # (rng_mode='device': the handle draws eps itself - the oracle then has nothing to say, and steps must be 0)
            self.eps_t = torch.as_tensor(self.eps, device=self.dev.device) if rng_mode == "inject" else None
            self.cond_t = torch.as_tensor(self.cond, device=self.dev.device) if inc else None
            tcsr = DeviceCSR.from_arrays(tip, tidx, tval, N, self.dev.device)
        for s in range(steps):
            e = r.standard_normal((R, c)).astype(np.float32)
            cd = (r.standard_normal((R, inc)) * 0.4).astype(np.float32) if inc else None
            lo, hi = tip[s * R], tip[(s + 1) * R]
            self.ora.partial_fit(tip[s * R:(s + 1) * R + 1] - lo, tidx[lo:hi], tval[lo:hi], e, [cd] if inc else None)
            if self.dev is not None:
                self.dev.vae_step(tcsr, s * R, R, cond=None if cd is None else torch.as_tensor(cd, device=self.dev.device), eps=e)

    def oracle_scores(self, n=None):
        n = self.rows if n is None else n
        end = self.ip[n]
        return self.ora.predict(self.ip[:n + 1], self.idx[:end], self.val[:end], self.eps[:n],
                                [self.cond[:n]] if self.inc else None)

    def topk(self, k, excl, lo=0, hi=None):
        """Rows [lo, hi) in calls of at most vae_rank_max_rows(k) rows (the library's contract; long lists take fewer rows)."""
        hi = self.rows if hi is None else hi
        cap, out = self.dev.vae_rank_max_rows(k), []
        for a in range(lo, hi, cap):
            b = min(a + cap, hi)
            out.append(self.dev.vae_predict_topk(self.csr, a, b - a, k, cond=None if self.cond_t is None else self.cond_t[a:b],
                                                 eps=None if self.eps_t is None else self.eps_t[a:b], exclude_known=excl))
        return torch.cat([o[0] for o in out]).cpu().numpy(), torch.cat([o[1] for o in out]).cpu().numpy()


def _check_lists(ids, vals, want_ids, want_vals, scaled, docs, k, excl, tol, what):
    n = ids.shape[0]
    err = float(np.abs(vals - want_vals).max())
    b, j = np.nonzero(ids != want_ids)
    pad = (ids[b, j] < 0) | (want_ids[b, j] < 0)
    gap = np.abs(scaled[b, np.maximum(ids[b, j], 0)] - scaled[b, np.maximum(want_ids[b, j], 0)])
    print(f"{what}: k={k} exclude_known={excl} rows={n} max |score diff|={err:.3g} positions that differ={len(b)}"
          f" their largest score gap={float(gap.max()) if len(b) else 0.0:.3g}")
    np.testing.assert_allclose(vals, want_vals, atol=tol, err_msg=what)
    assert not pad.any(), (what, "a padded position differs")
    assert np.all(gap <= tol), (what, len(b), float(gap.max()))
    for row in range(n):
        got = ids[row][ids[row] >= 0]
        n_ok = min(k, scaled.shape[1] - (len(docs[row]) if excl else 0))
        assert len(got) == n_ok and len(set(got.tolist())) == n_ok, (what, row)
        assert np.all(ids[row, n_ok:] == -1) and np.all(vals[row, n_ok:] == 0.0), (what, row)
        if excl:
            assert not (set(got.tolist()) & set(docs[row].tolist())), (what, row)


CASES = [  # N, h, c, inc, max_batch, rows, long row, [(k, exclude_known)]
    # the headline widths, a ragged last tile, 300 rows (beyond max_batch and beyond 224), row 5 names 2600 of the 3001 items
    (3001, 200, 50, 0, 100, 300, (5, 2600), [(1, True), (10, True), (20, True), (32, True), (33, True), (500, True), (1024, True),
                                               (10, False), (33, False)]),
    # a condition block, another width class, fewer rows than max_batch / exactly max_batch / more / beyond 224
    (2000, 100, 30, 7, 64, 260, None, [(10, True), (500, False)]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_vae_rank_matches_the_oracle_and_the_dense_form(case):
    """Ground truth: the float64 ranking of OracleVAE.predict's scores under the project's rule (known items dropped, better
    score first, then the smaller id).  Scaled scores within TOL; ids differ only where the two items' oracle scores lie
    within TOL; k distinct ids, no known item, -1 / 0 padding.  Then the same lists against aae_vae_predict per max_batch rows +
    the host pipeline at the 2e-6 bound of tests/test_rank_gpu.py."""
    N, h, c, inc, R, rows, long_row, ks = CASES[case]
    cs = Case(case, N, h, c, inc, R, rows, long_row=long_row)
    want = cs.oracle_scores()
    scaled = _scaled(want.astype(np.float64))
    full = np.concatenate([cs.dev.vae_predict(cs.csr, s, min(R, rows - s), cond=None if cs.cond_t is None else cs.cond_t[s:s + R],
                                              eps=cs.eps_t[s:s + R]).cpu().numpy() for s in range(0, rows, R)])
    print("aae_vae_predict against the oracle: max |diff| =", float(np.abs(full - want).max()))
    dscaled = _scaled(full.astype(np.float64))
    for k, excl in ks:
        assert cs.dev.vae_rank_max_rows(k) > R, (k, cs.dev.vae_rank_max_rows(k))
        for lo, hi in ([(0, rows)] if case == 0 else [(0, rows), (0, R - 24), (0, R), (0, R + 36)]):
            ids, vals = cs.topk(k, excl, lo, hi)
            want_ids, want_vals = _host_topk(want[lo:hi], cs.docs[lo:hi], k, excl)
            _check_lists(ids, vals, want_ids, want_vals, scaled[lo:hi], cs.docs[lo:hi], k, excl, TOL, f"oracle[{lo}:{hi}]")
            d_ids, d_vals = _host_topk(full[lo:hi], cs.docs[lo:hi], k, excl)
            _check_lists(ids, vals, d_ids, d_vals, dscaled[lo:hi], cs.docs[lo:hi], k, excl, 2e-6, f"dense[{lo}:{hi}]")
    # the decode form behind aae_vae_encode(train = 0): the same lists within the same bound
    k, excl = 10, True
    ids, vals = cs.topk(k, excl)
    z = torch.cat([cs.dev.vae_encode(cs.csr, s, min(R, rows - s), eps=cs.eps_t[s:s + R], train=False) for s in range(0, rows, R)])
    zc = z if cs.cond_t is None else torch.cat([z, cs.cond_t], 1)
    ids2, vals2 = cs.dev.vae_decode_topk(zc, cs.csr, 0, k, exclude_known=excl)
    _check_lists(ids2.cpu().numpy(), vals2.cpu().numpy(), ids, vals, dscaled, cs.docs, k, excl, 2e-6, "decode form")


def _truth(r, N, docs, per_row, known_share=0.0):
    """Held-out items: `per_row` per row that the row does not name (and, with known_share, some that it does)."""
    rows = []
    for d in docs:
        free = np.setdiff1d(np.arange(N), d)
        t = r.choice(free, size=min(per_row, len(free)), replace=False)
        if known_share and r.random() < known_share:
            t = np.concatenate([t, r.choice(d, size=1)])
        rows.append(np.sort(t))
    ip = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return ip, np.concatenate(rows).astype(np.int32), rows


def _oracle_ranks(scores, docs, truth_rows, excl, tol):
    """(ranks in CSR order, near-tie flags): the rank of every held-out item under the project's rule in float64, and whether
    another item's scaled score lies within tol of it (the entry is then left out of the comparison)."""
    ranks, near = [], []
    sc = _scaled(scores.astype(np.float64))
    for b, ts in enumerate(truth_rows):
        s = sc[b]
        known = np.zeros(s.size, dtype=bool)
        if excl:
            known[docs[b]] = True
        for t in ts:
            if known[t]:
                ranks.append(int((~known).sum()) + 1 + int(known[:t].sum()))
                near.append(False)
                continue
            better = (~known) & ((s > s[t]) | ((s == s[t]) & (np.arange(s.size) < t)))
            ranks.append(1 + int(better.sum()))
            d = np.abs(s - s[t])
            d[t] = np.inf
            near.append(bool((d <= tol).any()))
    return np.asarray(ranks, dtype=np.int64), np.asarray(near)


RANK_CASES = [(11, 600, 200, 50, 0, 100, 300), (12, 500, 100, 30, 7, 100, 260)]      # seed, N, h, c, inc, max_batch, rows


@pytest.mark.parametrize("case", range(len(RANK_CASES)))
def test_vae_ranks_match_the_k1024_lists_and_the_oracle(case):
    """aae_vae_predict_ranks: entry by entry the position in the same handle's k = min(1024, N) list where r <= that k (the
    contract of include/aaerec_hip.h for lists of k > 20), and the oracle's ranking wherever the held-out item's oracle score
    is farther than TOL from every other item's; the entries left out are counted and may be 2 % at most.  The vocabularies
    are small on purpose: N items spread over [0, 1] put another item within 1e-5 of a given one with probability ~2e-5 N, and
    the seeds were checked on the CPU with the oracle alone (Case(with_device=False)) to stay under the cap: 11 of 970 entries
    (1.1 %) at 600 items, 4 of 823 (0.5 %) at 500."""
    from aaerec._hip import DeviceCSR
    seed, N, h, c, inc, R, rows = RANK_CASES[case]
    cs = Case(seed, N, h, c, inc, R, rows, max_len=20)
    r = np.random.default_rng(seed)
    tip, tidx, truth_rows = _truth(r, N, cs.docs, 3, known_share=0.2)
    truth = DeviceCSR.from_arrays(tip, tidx, np.ones(len(tidx), dtype=np.float32), N, cs.dev.device)
    want = cs.oracle_scores()
    for excl in (True, False):
        got = cs.dev.vae_predict_ranks(cs.csr, 0, rows, truth, cond=cs.cond_t, eps=cs.eps_t, exclude_known=excl).cpu().numpy()
        k = min(1024, N)
        assert cs.dev.vae_rank_max_rows(k) >= rows and cs.dev.vae_rank_full_max_rows() >= rows      # (one call each: the same hidden activations)
        ids, _ = cs.topk(k, excl)
        pos = 0
        for b, ts in enumerate(truth_rows):
            for t in ts:
                rk = int(got[pos])
                pos += 1
                if rk <= k and ids[b, rk - 1] >= 0:
                    assert ids[b, rk - 1] == t, (b, t, rk)
                else:
                    assert t not in ids[b].tolist(), (b, t, rk)
        oranks, near = _oracle_ranks(want, cs.docs, truth_rows, excl, TOL)
        share = float(near.mean())
        print(f"ranks case {case} exclude_known={excl}: {len(got)} entries, {int(near.sum())} left out as near-ties ({share:.2%}),"
              f" {int((got[~near] != oranks[~near]).sum())} of the others differ")
        assert share <= NEAR_TIE_CAP, share
        np.testing.assert_array_equal(got[~near], oranks[~near])
        # the decode form: the same ranks from the caller-built decoder input
        z = torch.cat([cs.dev.vae_encode(cs.csr, s, min(R, rows - s), eps=cs.eps_t[s:s + R], train=False) for s in range(0, rows, R)])
        zc = z if cs.cond_t is None else torch.cat([z, cs.cond_t], 1)
        got2 = cs.dev.vae_decode_ranks(zc, cs.csr, 0, truth, exclude_known=excl).cpu().numpy()
        print("   decode form: entries that differ from the predict form:", int((got2 != got).sum()))
        assert np.array_equal(got2[~near], got[~near])


@pytest.mark.parametrize("rows,splits", [(160, [(0, 64), (64, 160)]), (160, [(0, 3), (3, 103), (103, 160)]),
                                         (520, [(0, 260), (260, 520)]), (520, [(0, 225), (225, 520)])])
def test_vae_rank_calls_agree_bitwise_however_the_rows_are_chunked(rows, splits):
    """A call of R rows == the concatenation of calls on a split of it on the same side of 224 rows, bit for bit, with the
    matching eps (and cond) slices: lists of k = 10, 32 and - where one call takes the rows: a long list keeps 8 K words a row
    in the workspace - k = 33, and the full ranks."""
    from aaerec._hip import DeviceCSR
    cs = Case(21, 1500, 64, 24, 5, 100, rows, max_len=12)
    r = np.random.default_rng(3)
    tip, tidx, truth_rows = _truth(r, cs.N, cs.docs, 2)
    truth = DeviceCSR.from_arrays(tip, tidx, np.ones(len(tidx), dtype=np.float32), cs.N, cs.dev.device)
    ks = [k for k in (10, 32, 33) if cs.dev.vae_rank_max_rows(k) >= rows]
    print("rows", rows, "caps", {k: cs.dev.vae_rank_max_rows(k) for k in (10, 32, 33)}, "full", cs.dev.vae_rank_full_max_rows())
    assert 10 in ks and 32 in ks and (33 in ks or rows > 224), ks
    assert cs.dev.vae_rank_full_max_rows() >= rows

    def one(k, lo, hi):
        ids, vals = cs.dev.vae_predict_topk(cs.csr, lo, hi - lo, k, cond=cs.cond_t[lo:hi], eps=cs.eps_t[lo:hi])
        return ids.cpu().numpy(), vals.cpu().numpy()
    for k in ks:
        ids, vals = one(k, 0, rows)
        parts = [one(k, lo, hi) for lo, hi in splits]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), ids), k
        assert np.array_equal(np.concatenate([p[1] for p in parts]).view(np.int32), vals.view(np.int32)), k
    whole = cs.dev.vae_predict_ranks(cs.csr, 0, rows, truth, cond=cs.cond_t, eps=cs.eps_t).cpu().numpy()
    parts = [cs.dev.vae_predict_ranks(cs.csr, lo, hi - lo, truth, cond=cs.cond_t[lo:hi], eps=cs.eps_t[lo:hi]).cpu().numpy()
             for lo, hi in splits]
    assert np.array_equal(np.concatenate(parts), whole)


def test_device_generator_with_zero_variance_equals_injected_zeros():
    """fc22.weight = 0, fc22.bias = -300: exp(-150) is 0 in fp32, so z = mu exactly whatever eps is drawn - a handle in
    rng_mode='device' must return exactly the lists and ranks of the injected path with eps = 0."""
    from aaerec._hip import HipAAE, DeviceCSR
    N, h, c, R, rows = 1200, 100, 30, 50, 120
    p = vae_params(N, h, c, 0, 31)
    p["fc22.weight"][:] = 0.0
    p["fc22.bias"][:] = -300.0
    r = np.random.default_rng(31)
    ip, idx, val, docs = _corpus(r, N, rows, 20)
    tip, tidx, _ = _truth(r, N, docs, 2)
    out = []
    for mode in ("device", "inject"):
        dev = HipAAE(N, h, c, max_batch=R, rng_mode=mode, seed=9, dropout=(0.0, 0.0), vae=True)
        dev.load_params(to_hip(p))
        csr = DeviceCSR.from_arrays(ip, idx, val, N, dev.device)
        truth = DeviceCSR.from_arrays(tip, tidx, np.ones(len(tidx), dtype=np.float32), N, dev.device)
        eps = None if mode == "device" else torch.zeros(rows, c, device=dev.device)
        res = []
        for k in (10, 40):
            assert dev.vae_rank_max_rows(k) >= rows > R, (k, dev.vae_rank_max_rows(k))
            ids, vals = dev.vae_predict_topk(csr, 0, rows, k, eps=eps)
            res += [ids.cpu().numpy(), vals.cpu().numpy().view(np.int32)]
        res.append(dev.vae_predict_ranks(csr, 0, rows, truth, eps=eps).cpu().numpy())
        out.append(res)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_reference_rng_mode_gives_the_top_k_of_predict():
    """rng_mode='reference': VAE.predict_topk draws eps as predict() draws it (torch.randn per batch_size rows, in row
    order), so with the same torch seed its lists are the top 10 of predict() under the tie rule, within the 2e-6 bound."""
    import scipy.sparse as sp
    from aaerec.vae import VAE
    rs = np.random.RandomState(4)
    N, n = 400, 330
    protos = [rs.choice(N, size=10, replace=False) for _ in range(25)]
    rows = [np.sort(rs.choice(protos[rs.randint(25)], size=rs.randint(3, 8), replace=False)) for _ in range(n)]
    X = sp.csr_matrix((np.ones(sum(map(len, rows)), dtype=np.float32), np.concatenate(rows),
                       np.concatenate([[0], np.cumsum([len(x) for x in rows])])), shape=(n, N))
    torch.manual_seed(1)
    np.random.seed(1)
    model = VAE(N, N, n_hidden=60, n_code=20, n_epochs=3, batch_size=50, lr=0.01, verbose=False, rng_mode="reference")
    model.fit(X[:200])
    Xt = X[200:]                                  # 130 rows: three draws of predict(), the last of 30 rows
    torch.manual_seed(5)
    ids, vals = model.predict_topk(Xt, k=10)
    torch.manual_seed(5)
    full = model.predict(Xt)
    docs = [Xt.indices[Xt.indptr[b]:Xt.indptr[b + 1]] for b in range(Xt.shape[0])]
    want_ids, want_vals = _host_topk(full, docs, 10, True)
    _check_lists(ids, vals, want_ids, want_vals, _scaled(full.astype(np.float64)), docs, 10, True, 2e-6, "reference rng")
    # the ranks of the held-out items: position r - 1 of the list where r <= 10
    Y = sp.csr_matrix((np.ones(len(docs), dtype=np.float32), ([*range(len(docs))], [int(want_ids[b, 2]) for b in range(len(docs))])),
                      shape=Xt.shape)
    torch.manual_seed(5)
    ranks = model.predict_ranks(Xt, Y)
    torch.manual_seed(5)
    ids32, _ = model.predict_topk(Xt, k=32)
    for b in range(len(docs)):
        assert ids32[b, ranks[b].data[0] - 1] == Y[b].indices[0]


def test_the_aae_calls_keep_what_they_did_and_the_vae_calls_refuse_another_handle():
    from aaerec._hip import HipAAE, DeviceCSR, AaeHipError
    N, h, c, R = 900, 64, 16, 40
    r = np.random.default_rng(2)
    ip, idx, val, docs = _corpus(r, N, R, 12)
    aae = HipAAE(N, h, c, max_batch=R, rng_mode="device", seed=1)
    csr = DeviceCSR.from_arrays(ip, idx, val, N, aae.device)
    with pytest.raises(AaeHipError):
        aae.vae_predict_topk(csr, 0, R, 10)
    with pytest.raises(AaeHipError):
        aae.vae_rank_max_rows(10)
    vae = HipAAE(N, h, c, max_batch=R, rng_mode="inject", dropout=(0.0, 0.0), vae=True)
    vae.load_params(to_hip(vae_params(N, h, c, 0, 3)))
    assert vae.rank_max_rows(10) == R and vae.rank_full_max_rows() == R       # the AAE calls on a VAE handle: the dense form, as before
    assert vae.vae_rank_max_rows(10) > R and vae.vae_rank_full_max_rows() > R
    with pytest.raises(AaeHipError):
        vae.vae_predict_topk(csr, 0, R, 10, eps=None)                          # inject mode needs eps
    # a handle without the fused rank kernels: the dense form (aae_vae_predict into the scratch, ranked there), max_batch rows
    import os
    os.environ["AAE_NO_RANK_FUSED"] = "1"
    try:
        old = HipAAE(N, h, c, max_batch=R, rng_mode="inject", dropout=(0.0, 0.0), vae=True)
    finally:
        del os.environ["AAE_NO_RANK_FUSED"]
    old.load_params(to_hip(vae_params(N, h, c, 0, 3)))
    assert old.vae_rank_max_rows(10) == R and old.vae_rank_full_max_rows() == R
    eps = torch.as_tensor(r.standard_normal((R, c)).astype(np.float32), device=vae.device)
    for k in (10, 40):
        ids, vals = vae.vae_predict_topk(csr, 0, R, k, eps=eps)
        ids2, vals2 = old.vae_predict_topk(csr, 0, R, k, eps=eps)
        full = old.vae_predict(csr, 0, R, eps=eps).cpu().numpy()
        _check_lists(ids.cpu().numpy(), vals.cpu().numpy(), ids2.cpu().numpy().astype(np.int64), vals2.cpu().numpy(),
                     _scaled(full.astype(np.float64)), docs, k, True, 2e-6, "fused against the dense form")
    with pytest.raises(AaeHipError):
        old.vae_predict_topk(csr, 0, R + 1, 10, eps=torch.zeros(R + 1, c, device=vae.device))      # beyond max_batch: refused


def test_vae_ranks_are_the_positions_in_a_1024_entry_list_over_many_tiles():
    """The contract of include/aaerec_hip.h without the oracle: on the 3001-item vocabulary (94 tiles, a ragged last one, a row
    that names most of it) every rank r <= 1024 of aae_vae_predict_ranks is position r - 1 of the same handle's k = 1024 list,
    and an item of a larger rank (or a known one) is not in the list."""
    from aaerec._hip import DeviceCSR
    N, rows, k = 3001, 300, 1024
    cs = Case(0, N, 200, 50, 0, 100, rows, long_row=(5, 2600))
    r = np.random.default_rng(8)
    tip, tidx, truth_rows = _truth(r, N, cs.docs, 4, known_share=0.2)
    truth = DeviceCSR.from_arrays(tip, tidx, np.ones(len(tidx), dtype=np.float32), N, cs.dev.device)
    assert cs.dev.vae_rank_max_rows(k) >= rows and cs.dev.vae_rank_full_max_rows() >= rows
    for excl in (True, False):
        got = cs.dev.vae_predict_ranks(cs.csr, 0, rows, truth, eps=cs.eps_t, exclude_known=excl).cpu().numpy()
        ids, _ = cs.topk(k, excl)
        pos = inside = 0
        for b, ts in enumerate(truth_rows):
            for t in ts:
                rk = int(got[pos])
                pos += 1
                if rk <= k and ids[b, rk - 1] >= 0:
                    inside += 1
                    assert ids[b, rk - 1] == t, (b, t, rk)
                else:
                    assert t not in ids[b].tolist(), (b, t, rk)
        print(f"exclude_known={excl}: {pos} held-out items, {inside} of them inside the 1024-entry lists")
        assert 0 < inside < pos


@pytest.mark.parametrize("inc", [0, 7])
def test_overflowing_collect_lists_are_ranked_again_with_their_own_eps_rows(inc):
    """RANK_COLLECT_CAP set to a handful of entries: every row of a k > 32 call overflows and is ranked again through the score
    matrix, in spans of max_batch rows - 150 rows on a handle of 64, so spans start at rows 64 and 128 and a wrong eps / cond /
    output offset would show.  The lists must be those of the uncapped handle (2e-6 rule) and of the oracle (TOL), in the
    predict and in the decode form; rank_long_stats counts the rows."""
    from aaerec import _hip
    N, h, c, R, rows, k = 2000, 100, 30, 64, 150, 100
    _hip.set_option("RANK_COLLECT_CAP", 8)
    try:
        small = Case(40 + inc, N, h, c, inc, R, rows)
    finally:
        _hip.set_option("RANK_COLLECT_CAP", None)
    plain = Case(40 + inc, N, h, c, inc, R, rows)
    assert min(small.dev.vae_rank_max_rows(k), plain.dev.vae_rank_max_rows(k)) >= rows > 2 * R
    ids, vals = plain.topk(k, True)
    st = plain.dev.rank_long_stats()
    assert st["calls"] == 1 and st["overflow_rows"] == 0, st
    ids_s, vals_s = small.topk(k, True)
    st = small.dev.rank_long_stats()
    assert st["calls"] == 1 and st["overflow_rows"] == rows, st
    want = small.oracle_scores()
    scaled = _scaled(want.astype(np.float64))
    want_ids, want_vals = _host_topk(want, small.docs, k, True)
    _check_lists(ids_s, vals_s, want_ids, want_vals, scaled, small.docs, k, True, TOL, "overflow against the oracle")
    _check_lists(ids_s, vals_s, ids.astype(np.int64), vals, scaled, small.docs, k, True, 2e-6, "overflow against the uncapped handle")
    z = torch.cat([small.dev.vae_encode(small.csr, s, min(R, rows - s), eps=small.eps_t[s:s + R], train=False) for s in range(0, rows, R)])
    zc = z if small.cond_t is None else torch.cat([z, small.cond_t], 1)
    ids_d, vals_d = (t.cpu().numpy() for t in small.dev.vae_decode_topk(zc, small.csr, 0, k))
    st = small.dev.rank_long_stats()
    assert st["calls"] == 1 and st["overflow_rows"] == rows, st
    _check_lists(ids_d, vals_d, want_ids, want_vals, scaled, small.docs, k, True, TOL, "overflow, decode form, against the oracle")
    _check_lists(ids_d, vals_d, ids.astype(np.int64), vals, scaled, small.docs, k, True, 2e-6, "overflow, decode form")


def test_device_generator_draws_what_vae_predict_draws():
    """rng_mode='device' with the variance the initialisation gives (std ~ 1): the 4-row kernel's reparametrisation must draw, for
    (seed, step, row of the call, column), what chain.h's op draws in aae_vae_predict.  Rows <= max_batch: the lists are the top k
    of vae_predict on the same handle at the same step (2e-6 rule).  And the row offset: with every list overflowing, the spans
    that start at rows 64 and 128 are ranked again with the generator rows counted from there - the lists of the uncapped
    handle (same seed, same step), whose one fused call drew rows 0 .. 149."""
    from aaerec import _hip
    N, h, c, R, rows = 2000, 100, 30, 64, 150
    cs = Case(50, N, h, c, 0, R, rows, steps=0, rng_mode="device")
    full = cs.dev.vae_predict(cs.csr, 0, R).cpu().numpy()
    injected_zero = cs.dev.vae_predict(cs.csr, 0, R, eps=torch.zeros(R, c, device=cs.dev.device)).cpu().numpy()
    assert np.abs(full - injected_zero).max() > 1e-2          # (the draw matters: a wrong one cannot hide)
    dscaled = _scaled(full.astype(np.float64))
    for k in (10, 32, 40):
        ids, vals = cs.topk(k, True, 0, R)
        want_ids, want_vals = _host_topk(full, cs.docs[:R], k, True)
        _check_lists(ids, vals, want_ids, want_vals, dscaled, cs.docs[:R], k, True, 2e-6, "device generator against vae_predict")
    _hip.set_option("RANK_COLLECT_CAP", 8)
    try:
        small = Case(50, N, h, c, 0, R, rows, steps=0, rng_mode="device")
    finally:
        _hip.set_option("RANK_COLLECT_CAP", None)
    k = 100
    assert min(small.dev.vae_rank_max_rows(k), cs.dev.vae_rank_max_rows(k)) >= rows
    cs.dev.rank_long_stats()
    ids, vals = cs.topk(k, True)
    assert cs.dev.rank_long_stats()["overflow_rows"] == 0
    ids_s, vals_s = small.topk(k, True)
    assert small.dev.rank_long_stats()["overflow_rows"] == rows
    # (scaled scores of the first max_batch rows locate the gaps; beyond them the uncapped lists' own scores do)
    np.testing.assert_allclose(vals_s, vals, atol=2e-6)
    d = ids_s != ids
    assert np.all(np.abs(vals_s[d] - vals[d]) <= 2e-6), int(d.sum())
    print("device generator through the overflow path: positions that differ from the uncapped handle's:", int(d.sum()))

"""The truncated-SVD baseline on the device (csrc/lowrank.h, csrc/abi_lowrank.h, aaerec/lowrank.py) against the float64
definition under the acceptance rule of tests/lowrank_cases.py (c = 1: the reconstruction runs on the fp32 matrix pipe).

Shapes where the kernels can go wrong, not workload size: 1003 items (no multiple of 4 or 64) + 37 title features; dims 1, 3,
10, 100, 260 (below, at and off the GEMM's 16-deep slabs, one and two waves of the projection); 1, 70, 257 rows (across the
64-row tile); an empty row, a row naming all but two items, a row of 3000 entries (twelve LDS pieces of the projection).
tests/test_lowrank_cpu.py asserts the ambiguity cap of every case and the fixture's freedom from ambiguity."""
import numpy as np
import pytest
import scipy.sparse as sp

import lowrank_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", params=range(len(LC.GPU_CASES)), ids=["dims%d-rows%d" % c[:2] for c in LC.GPU_CASES])
def case(request):
    """One generated case with its float64 reference and its device objects: built once, read by every test."""
    from aaerec import _hip
    c = LC.gpu_case(*LC.GPU_CASES[request.param])
    ip, idx, val = c["raw"]
    c["lr"] = _hip.DeviceLowRank(c["V"], DEV)
    c["feat"] = _hip.DeviceCSR.from_arrays(ip, idx, val, LC.N_FEATURES, DEV)       # (raw: the 3000-entry row keeps its duplicates)
    c["items"], c["truth"] = _hip.DeviceCSR(c["X"], DEV), _hip.DeviceCSR(c["Y"], DEV)
    for a in (c["ref"]["S"], c["ref"]["tol"]):
        a.setflags(write=False)
    return c


def test_scores_within_the_bound_of_the_float64_product(case):
    import torch
    from aaerec import _hip
    S, tol, n = case["ref"]["S"], case["ref"]["tol"], case["rows"]
    got = _hip.lowrank_scores(case["lr"], LC.N_ITEMS, case["feat"], 0, n).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (n, LC.N_ITEMS)
    err = np.abs(got.astype(np.float64) - S)
    print("dims", case["dims"], "rows", n, "max err / tol", float((err / np.maximum(tol, 1e-300)).max()), "max err", float(err.max()))
    assert (err <= tol).all()
    if n > 3:
        assert (got[1] == 0).all()                                      # the empty row
    assert (got[:, list(LC.ZERO_ITEMS)] == 0).all()                     # items never seen: exact zeros
    # a window of the rows into a caller's wider matrix: nothing is written beyond n_items; the same bits
    lo, m = min(2, n - 1), min(9, n - min(2, n - 1))
    out = torch.full((m, LC.N_ITEMS + 5), -7.0, dtype=torch.float32, device=DEV)
    part = _hip.lowrank_scores(case["lr"], LC.N_ITEMS, case["feat"], lo, m, out=out).cpu().numpy()
    assert part.tobytes() == got[lo:lo + m].tobytes() and (out[:, LC.N_ITEMS:] == -7.0).all()
    # rows named through rows_dev, in permuted order
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    again = _hip.lowrank_scores(case["lr"], LC.N_ITEMS, case["feat"], 0, n, rows=torch.as_tensor(perm).to(DEV)).cpu().numpy()
    assert again.tobytes() == got[perm].tobytes()


@pytest.mark.parametrize("k", LC.GPU_KS)
def test_topk_under_the_acceptance_rule(case, k):
    from aaerec import _hip
    ids, val = _hip.lowrank_topk(case["lr"], LC.N_ITEMS, case["feat"], case["items"], 0, case["rows"], k)
    LC.check_topk(case["ref"], case["X"], ids.cpu().numpy(), val.cpu().numpy(), k)


def test_ranks_under_the_acceptance_rule(case):
    from aaerec import _hip
    Y = case["Y"]
    ranks = _hip.lowrank_ranks(case["lr"], LC.N_ITEMS, case["feat"], case["items"], 0, case["rows"], case["truth"], Y.nnz).cpu().numpy()
    assert ranks.dtype == np.int32 and ranks.shape == (Y.nnz,)
    LC.check_ranks(case["ref"], case["X"], Y, ranks)
    # an entry of rank r <= 500 is position r - 1 of the list of 500: both come from the same scores
    ids = _hip.lowrank_topk(case["lr"], LC.N_ITEMS, case["feat"], case["items"], 0, case["rows"], 500)[0].cpu().numpy()
    e = 0
    for i in range(case["rows"]):
        for t in Y.indices[Y.indptr[i]:Y.indptr[i + 1]]:
            if ranks[e] <= 500 and ids[i, ranks[e] - 1] >= 0:
                assert ids[i, ranks[e] - 1] == t
            e += 1


def test_two_calls_give_identical_bits(case):
    from aaerec import _hip
    n = case["rows"]
    a = _hip.lowrank_scores(case["lr"], LC.N_ITEMS, case["feat"], 0, n).cpu().numpy()
    b = _hip.lowrank_scores(case["lr"], LC.N_ITEMS, case["feat"], 0, n).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    one = [t.cpu().numpy() for t in _hip.lowrank_topk(case["lr"], LC.N_ITEMS, case["feat"], case["items"], 0, n, 33)]
    two = [t.cpu().numpy() for t in _hip.lowrank_topk(case["lr"], LC.N_ITEMS, case["feat"], case["items"], 0, n, 33)]
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()


def _model(c, scratch_bytes):
    from aaerec.lowrank import SVDRecommender
    rec = SVDRecommender(c["dims"], scratch_bytes=scratch_bytes, device=DEV)
    rec.svd.components_ = c["V"]                       # (recorded components: the device table is derived when first needed)
    rec.n_classes = LC.N_ITEMS
    return rec


def test_chunking_gives_identical_ids_scores_and_ranks():
    c = LC.gpu_case(*LC.GPU_CASES[4])                  # dims 260, 257 rows
    n, row_bytes = c["rows"], 4 * ((LC.N_ITEMS + 3) & ~3)
    test = LC.Titled(c["F"])
    outs = []
    for chunks, scratch in ((1, 256 << 20), (3, 86 * row_bytes), (257, row_bytes)):
        rec = _model(c, scratch)
        assert rec.on_device(500) and -(-n // rec._chunk_rows(LC.N_ITEMS)) == chunks
        ids, val = rec.predict_topk(test, k=100)
        ranks = rec.predict_ranks(test, c["Y"])
        outs.append((ids.tobytes(), val.tobytes(), ranks.data.tobytes()))
    assert outs[0] == outs[1] == outs[2]
    # and they are the acceptance rule's lists (canonical rows: the 3000 entries summed to their distinct ids)
    ref = LC.reference(c["V"], c["F"], c["X"])
    LC.check_topk(ref, c["X"], ids, val, 100)
    LC.check_ranks(ref, c["X"], c["Y"], ranks.data)


def test_out_of_table_ids_are_skipped():
    from aaerec import _hip
    c = LC.gpu_case(*LC.GPU_CASES[3])                  # dims 100, 70 rows
    ip, idx, val = (a.copy() for a in c["raw"])
    lo = int(ip[6])
    assert ip[7] - lo >= 3
    F = sp.csr_matrix((val.astype(np.float64), idx, ip), shape=(c["rows"], LC.N_FEATURES)).tolil()
    for j in idx[lo:lo + 2]:
        F[6, j] = 0                                    # the definition without the two entries
    idx[lo], idx[lo + 1] = LC.N_FEATURES + 5, -1       # ... whose ids leave the table
    bad = _hip.DeviceCSR.from_arrays(ip, idx, val, LC.N_FEATURES, DEV)
    lr = _hip.DeviceLowRank(c["V"], DEV)
    got = _hip.lowrank_scores(lr, LC.N_ITEMS, bad, 6, 1).cpu().numpy().astype(np.float64)
    ref = LC.reference(c["V"], sp.csr_matrix(F)[6], c["X"][6], nnz=[ip[7] - lo])
    assert (np.abs(got - ref["S"]) <= ref["tol"]).all() and np.abs(ref["S"]).max() > 0


def _bags(fx):
    from aaerec.datasets import Bags
    z = fx["z"]
    ip, tok = z["doc_indptr"], z["doc_tokens"]
    owners = ["d%d" % i for i in range(ip.size - 1)]
    data = [["i%d" % t for t in tok[ip[i]:ip[i + 1]]] for i in range(ip.size - 1)]
    return Bags(data, owners, {"year": dict(zip(owners, z["doc_years"].tolist())), "title": dict(zip(owners, z["doc_titles"].tolist()))})


def _recorded_draw(ev, fx):
    """The split is the one the reference made when the components were recorded: the same training matrix and the same test
    bags.  WHICH item of a test bag is held out the reference draws from an unordered set (datasets.py:105), this package from
    the sorted one: the recorded draw is put in place of this run's."""
    assert (ev.train_set.tocsr() != fx["train"]).nnz == 0
    assert ((sp.csr_matrix(ev.x_test) + sp.csr_matrix(ev.y_test)) != (fx["test"] + fx["truth"])).nnz == 0
    X = fx["test"]
    ev.test_set.data = [X.indices[X.indptr[i]:X.indptr[i + 1]].tolist() for i in range(X.shape[0])]
    ev.x_test, ev.y_test = fx["test"].copy(), fx["truth"].copy()
    assert (ev.test_set.tocsr() != fx["test"]).nnz == 0


@pytest.mark.parametrize("metrics", [["mrr@10", "map@10", "p@5", "mrr@20"], ["mrr", "map", "mrr@10"]])
@pytest.mark.parametrize("name", ["svd_plain", "svd_titles"])
def test_evaluation_takes_the_device_route_and_gives_the_dense_numbers(name, metrics):
    from aaerec import evaluation as E
    fx = LC.load_fixture(name)
    z = fx["z"]
    Recorded = LC.recorded_class(fx["components"])
    results = {}
    for topk in (True, False):
        ev = E.Evaluation(_bags(fx), int(z["split_year"]), metrics=metrics, logfile=None, topk=topk)
        ev.setup(seed=int(z["setup_seed"]), min_elements=int(z["min_elements"]), drop=int(z["drop"]))
        _recorded_draw(ev, fx)
        rec = Recorded(fx["dims"], use_title=fx["use_title"], random_state=fx["random_state"], device=DEV)
        asked = []
        real = rec.predict
        rec.predict = lambda *a, **kw: (asked.append("predict"), real(*a, **kw))[1]
        results[topk] = np.asarray(ev([rec])[0], dtype=np.float64)
        assert (asked == []) == topk and rec.on_device(20)
    print(name, metrics, results[True].ravel().tolist(), results[False].ravel().tolist())
    assert results[False][:, 0].min() > 0.05                   # the split is one the baseline can answer
    np.testing.assert_allclose(results[True], results[False], rtol=0, atol=1e-12)

"""Random baseline with seeded draws and its ranking on the device (the reference's RandomBaseline, baselines.py:7-19).

The reference's `predict` is `numpy.random.rand(rows, items)` from numpy's global generator: nothing to reproduce, and a float64
matrix of the test set's shape (8 GB for 10 000 rows at 100 000 items) that Evaluation scales, masks and arg-partitions on the
host.  With a `seed` the scores come from the library's keyed generator instead (csrc/device_common.h rng_key / hash_cell, stream
15), one definition for host and device:

    key    = rng_key(seed, draw, 0) ^ 15 * 0xA0761D6478BD642F
    s(r,j) = hash_cell(key, r, j) >> (32 - bits)              an integer in [0, 2^bits); bits = 24 in the class
    score  = s * 2^-bits                                      exact in float32

for item j of row r of the WHOLE test set and a draw number `draw` >= 0 (another draw: another block of scores under the same
seed).  The same seed then gives the same floor line under every table of results, on every route, however the rows are chunked.
`draw_scores` is that definition in NumPy.  csrc/randrank.h ranks without ever storing a score: a list is an exact radix select
over the regenerated draws, the ranks of the held-out items are counted while the draws go by.  The ordering is the project's one
rule (aaerec/ranking.py): the larger score first, THE SMALLER ID AT EQUAL SCORES (24-bit values tie in nearly every row of
100 000 items), known items left out.  Scaled scores are the min-max scaling over all items of the row, known ones included -
what remove_non_missing gives on the dense matrix - with the fp32 formula of the other baselines (cooc._scaled).

Routes with a seed: the device where one is named and present, k <= min(1024, items) and no row holds more than 4096 held-out
items (`route` says "device" or None); the host route - `draw_scores` into `ranking.host_topk` / `host_ranks`, a block of rows at
a time - answers everything else with the same bits.  Without a seed (`seed=None`, the default) the class is the reference's:
`predict` is its line, and `predict_topk` / `predict_ranks` rank `numpy.random.rand` blocks on the host - NOT reproducible unless
the caller seeds numpy, and not the same numbers as ranking one `predict` matrix (the blocks are drawn as they are ranked).

`metrics=` (what Evaluation(metrics_on="device") asks for) leaves lists and ranks on the device and has the per-row metric values
formed there; the (mean, std) over the rows is numpy's, as on the host route (ranking.rank_metrics, reduce_on="host": [metrics,
rows] doubles come back, no CSR) - a floor line is the same pair to the bit whichever route and whichever metrics_on produced it.

This module is not `aaerec.baselines`: that name keeps resolving to the user's checkout of the reference (aaerec/__init__.py).
"""
import numpy as np
import torch
from numpy.random import rand

from . import _hip, ranking
from .base import Recommender
from .cooc import INT32_LIMIT, _scaled

_M64 = (1 << 64) - 1
STREAM = 15                                   # the generator's stream of this baseline (12-14 and 100 are taken)
BITS = _hip.RAND_BITS
_PREDICT_BLOCK_BYTES = 256 << 20              # device rows of one predict() download


def _key(seed, draw):
    """rng_key(seed, draw, 0) ^ STREAM * 0xA0761D6478BD642F as a Python int (64 bit)."""
    return ((int(seed) & _M64) ^ ((int(draw) * 0xD1B54A32D192ED03) & _M64) ^ ((STREAM * 0xA0761D6478BD642F) & _M64)) & _M64


def draw_values(seed, draw, row0, n_rows, n_items, bits=BITS):
    """uint32 [n_rows, n_items]: s(r, j) for rows [row0, row0 + n_rows) - hash_cell's two multiply-xorshift rounds over the key
    halves offset by odd multiples of row and item, modulo 2^32 throughout, then the top `bits` bits."""
    if not 1 <= bits <= 24:
        raise ValueError("bits must be in [1, 24]")
    if draw < 0 or row0 < 0 or n_rows < 0 or n_items < 0:
        raise ValueError("draw, row0, n_rows and n_items must not be negative")
    key = _key(seed, draw)
    r = ((np.arange(n_rows, dtype=np.uint64) + np.uint64(row0)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c = np.arange(n_items, dtype=np.uint64).astype(np.uint32)
    with np.errstate(over="ignore"):
        a = np.uint32(key & 0xFFFFFFFF) + r * np.uint32(0x9E3779B1)
        b = np.uint32(key >> 32) + c * np.uint32(0x85EBCA77)
        x = a[:, None] ^ b[None, :]
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x >> np.uint32(32 - bits)


def draw_scores(seed, draw, row0, n_rows, n_items, bits=BITS):
    """float32 [n_rows, n_items]: the scores of rows [row0, row0 + n_rows) of the test set, s * 2^-bits (exact)."""
    return draw_values(seed, draw, row0, n_rows, n_items, bits).astype(np.float32) * np.float32(2.0 ** -bits)


class RandomBaseline(Recommender):
    """Random Baseline.  seed: None for the reference's numpy.random.rand, or the seed of the keyed generator (the module
    docstring).  device: where seeded lists and ranks are formed; None keeps everything on the host, with the same bits."""

    bits = BITS               # bits of a draw; an instance may lower it (fewer bits: more ties), every route follows

    def __init__(self, seed=None, device="cuda:0"):
        super().__init__()
        self.seed = seed
        self.device = device

    def __str__(self):
        return "RNDM baseline"

    def train(self, X):
        pass

    def _on_device(self):
        return self.seed is not None and self.device is not None and torch.cuda.is_available()

    def predict(self, X, draw=0):
        X = X.tocsr()
        n, items = X.shape
        if self.seed is None:
            return rand(n, items)
        if not self._on_device() or not n or not items or items >= INT32_LIMIT:
            return draw_scores(self.seed, draw, 0, n, items, self.bits)
        out = np.empty((n, items), dtype=np.float32)
        block = max(1, _PREDICT_BLOCK_BYTES // (4 * ((items + 3) & ~3)))
        buf = None
        for start, rows in ranking.row_chunks(n, block):
            buf = _hip.rand_scores(self.seed, draw, start, rows, items, self.device, bits=self.bits, out=buf)
            out[start:start + rows] = buf[:rows, :items].cpu().numpy()
        return out

    # ---- ranking ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _inputs(test_set):
        X = test_set.tocsr()
        X.sum_duplicates()
        X.sort_indices()
        return X

    def _route_of(self, shape, k=None, Ys=None):
        n, items = shape
        if not self._on_device() or not n or not 1 <= items < INT32_LIMIT or n >= INT32_LIMIT:
            return None
        if k is not None and not 1 <= k <= min(_hip.RANK_K_MAX, items):
            return None
        if Ys is not None and Ys.shape[0] and int(np.diff(Ys.indptr).max()) > _hip.RAND_TRUTH_MAX:
            return None
        return "device"

    def route(self, test_set, k=None, y_true=None):
        """Which route predict_topk(test_set, k) - or, without k, predict_ranks(test_set, y_true) - takes: "device", or None on
        the host."""
        X = self._inputs(test_set)
        Ys = None if y_true is None else ranking.canonical_truth(y_true, X.shape, "the test set")
        return self._route_of(X.shape, k, Ys)

    def _host_rows(self, X, draw):
        n, items = X.shape
        if self.seed is None:
            return ranking.host_rows(X, lambda r0, r1: rand(min(r1, n) - r0, items))
        return ranking.host_rows(X, lambda r0, r1: draw_scores(self.seed, draw, r0, min(r1, n) - r0, items, self.bits))

    def predict_topk(self, test_set, k=10, y_true=None, metrics=None, draw=0):
        """(item ids int32 [n, k], scaled scores float32 [n, k]) of the k best new items per test bag under draw number `draw`:
        predict -> remove_non_missing -> argtopk; id -1 / score 0 behind a row's last rankable item.  metrics: a list of bounded
        metric names - [(mean, std)] per name against y_true comes back instead (ranking.rank_metrics on the device route).
        Without a seed the scores are numpy.random.rand blocks: not reproducible."""
        X = self._inputs(test_set)
        n, items = X.shape
        if k < 1:
            raise ValueError("k must be positive")
        if not self._route_of(X.shape, k):
            return ranking.host_finish_lists(ranking.host_topk(self._host_rows(X, draw), n, k, _scaled), metrics, y_true, X.shape)
        parts = [_hip.rand_topk(self.seed, draw, 0, items, _hip.DeviceCSR(X, self.device), 0, n, k, bits=self.bits)]
        return ranking.finish_lists(parts, k, metrics, y_true, X.shape, reduce_on="host")

    def predict_ranks(self, test_set, y_true, metrics=None, draw=0):
        """CSR of int32 with y_true's (canonical) pattern: the 1-based rank of every held-out item in the full ranking of its
        test bag, in predict_topk's ordering.  A held-out item that is a known item ranks behind every rankable one, among
        the known items by id.  metrics: a list of metric names - [(mean, std)] per name comes back instead."""
        X = self._inputs(test_set)
        n, items = X.shape
        Ys = ranking.canonical_truth(y_true, X.shape, "the test set")
        if not self._route_of(X.shape, None, Ys):
            return ranking.host_finish_ranks(ranking.host_ranks(self._host_rows(X, draw), Ys), metrics)
        csr, truth = _hip.DeviceCSR(X, self.device), _hip.DeviceCSR(Ys, self.device)
        return ranking.finish_ranks([_hip.rand_ranks(self.seed, draw, 0, items, csr, 0, n, truth, int(Ys.nnz), bits=self.bits)], Ys, metrics,
                                    reduce_on="host")
